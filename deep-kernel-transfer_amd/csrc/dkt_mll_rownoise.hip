// dkt_mll_rownoise_f32 / dkt_dirichlet_proba_f32 (include/dkt_abi.h; docs/DIRICHLET.md): the exact-GP marginal likelihood of B x C problems
// K = sv_c E + diag(noise_rows_c) -- a noise per ROW, what a Dirichlet classification likelihood makes of the class labels -- and the class
// probabilities of its latent posterior.
//
// TWO kernel instances, 256 threads each, plain fp32 on the VALU (the choice against the fp32 MFMA route of dkt_mll_mfma.hip: docs/DIRICHLET.md).
// rownoise_kernel, pass 0: a workgroup per (episode, class).  ONE (N + 1) x (N|1) matrix in LDS (64 KiB + 2.5 KiB of vectors at N = 127: two workgroups
// per CU).  Rows 0 .. N-1 hold the lower triangle of K, row N holds r = y - mean: the right-looking Cholesky sweep that turns the rows into L turns row N
// into t = L^-1 r, the forward substitution, at no barrier of its own.  logp = -1/2 t.t - sum log L_ii - N/2 log 2 pi.  Then, as in
// dkt_laplace_grad.hip, the inverse inside the factor's own storage: U = L^-T row by row into the upper triangle, alpha = U t, K^-1 = U U^T back over
// the lower triangle (its diagonal apart), G = 1/2 (alpha alpha^T - K^-1) written straight from it.  No jitter ladder: a pivot that is not finite and
// positive ends the problem (info, NaN outputs).  A shared E (class stride 0) has its classes summed by pass 1 of the SAME kernel (an element per
// thread, the classes in index order) from the per-class matrices pass 0 left in the workspace: no atomics, and the sum of a shared call is bit for
// bit the sum of the per-class call's outputs.  Every reduction has a fixed order that depends on nothing but N.
// dirichlet_proba_kernel: a group of W = 2^ceil(log2 C) lanes per query, a lane per class; max and sum over the classes by xor butterflies inside
// the group, the samples in index order (a compensated sum).
#include "dkt_laplace_lds.h"

namespace {

using namespace dkt_laplace;             // kWave, padded, wave_sum, cholesky_lower_rows, set_lds
constexpr int kT = 256;
constexpr int kVec = 128;
constexpr int kVecs = 5;                 // sd .. sred below
constexpr float kHalfLog2Pi = 0.918938533204672742f;

inline size_t rownoise_lds_bytes(int N) { return ((size_t)(N + 1) * padded(N) + kVecs * kVec) * sizeof(float); }

__global__ __launch_bounds__(kT) void rownoise_kernel(const float* __restrict__ E, long ebs, long ecs, const float* __restrict__ Y, long ybs,
                                                     const float* __restrict__ NR, long nbs, const float* __restrict__ sv,
                                                     const float* __restrict__ mean, const float* __restrict__ cw, float* __restrict__ logp,
                                                     float* __restrict__ alpha, float* __restrict__ Gout, float* __restrict__ dE,
                                                     float* __restrict__ dsv, float* __restrict__ dmean, float* __restrict__ chol,
                                                     int* __restrict__ info, int B, int C, int N, unsigned flags, int pass) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int NN = N * N;
    if (pass == 1) {
        // dE[b] = sum_c Gout[b, c], the classes in index order
        const long e = (long)blockIdx.x * kT + tid;
        if (e < (long)B * NN) {
            const long b = e / NN, r = e - b * NN;
            const float* src = Gout + b * C * (long)NN + r;
            float acc = src[0];
            for (int c = 1; c < C; ++c) acc += src[(long)c * NN];
            dE[e] = acc;
        }
        return;
    }
    const int NP = padded(N);
    float* sA = lds;                     // K (lower) + r (row N) -> L (strict lower) + t (row N) -> U = L^-T (upper, diagonal included) -> K^-1 (strict lower)
    float* sd = sA + (N + 1) * NP;       // pivots of L
    float* st = sd + kVec;               // t = L^-1 r
    float* sa = st + kVec;               // alpha
    float* sr = sa + kVec;               // diagonal of K^-1
    float* sred = sr + kVec;             // cross-wave partials
    const int lane = tid & (kWave - 1), wave = tid >> 6;
    const long prob = blockIdx.x;
    const int b = (int)(prob / C), c = (int)(prob % C);
    const float* Ep = E + (long)b * ebs + (long)c * ecs;
    const float* Yp = Y + (long)b * ybs + (long)c * N;
    const float* Np = NR + (long)b * nbs + (long)c * N;
    const float sc = sv[c], mu = mean[c];
    const float wc = cw ? cw[c] : 1.f;
    const bool grad = flags & DKT_MLL_WANT_GRAD;
    float* Gp = Gout + prob * (long)NN;

    for (int idx = tid; idx < NN; idx += kT) {
        int i = idx / N, j = idx - i * N;
        if (j <= i) sA[i * NP + j] = sc * Ep[idx] + (i == j ? Np[i] : 0.f);
    }
    if (tid < N) sA[N * NP + tid] = Yp[tid] - mu;
    __syncthreads();
    // the Cholesky sweep over the N + 1 rows; a bad pivot ends it for the whole workgroup
    const int bad = cholesky_lower_rows<kT, true>(sA, sd, N, N + 1, NP, tid);
    if (tid == 0) info[prob] = bad;
    if (bad) {
        const float nan = __builtin_nanf("");
        if (tid == 0) {
            logp[prob] = nan;
            if (grad && dsv) dsv[prob] = nan;
            if (grad && dmean) dmean[prob] = nan;
        }
        if (tid < N) alpha[prob * N + tid] = nan;
        for (int idx = tid; idx < NN; idx += kT) {
            if (grad) Gp[idx] = nan;
            if (flags & DKT_MLL_WANT_CHOL) chol[prob * (long)NN + idx] = nan;
        }
        return;
    }
    if (flags & DKT_MLL_WANT_CHOL) {
        float* Lp = chol + prob * (long)NN;
        for (int idx = tid; idx < NN; idx += kT) {
            int i = idx / N, j = idx - i * N;
            Lp[idx] = j < i ? sA[i * NP + j] : (j == i ? sd[i] : 0.f);
        }
    }
    // logp = -1/2 t.t - sum log L_ii - N/2 log 2 pi
    if (tid < N) {
        const float t = sA[N * NP + tid];
        st[tid] = t;
        sr[tid] = -0.5f * t * t - logf(sd[tid]);
        sA[tid * NP + tid] = 1.f / sd[tid];                       // U_ii
    }
    __syncthreads();
    {
        const float lp = wave_sum((lane < N ? sr[lane] : 0.f) + (lane + kWave < N ? sr[lane + kWave] : 0.f));
        if (tid == 0) logp[prob] = lp - (float)N * kHalfLog2Pi;
    }
    // U = L^-T into the upper triangle, row i of L^-1 at a time: U_ji = -(sum_{k=j}^{i-1} L_ik U_jk) / L_ii, j < i.  Thread j owns row j of U: it reads
    // its own earlier writes and the rows of L, which nobody writes -- no barrier inside.  The k loop is the same for every lane (guarded, not started at
    // the lane's own j): the lanes read sA[j * NP + k], NP words apart (odd: every bank once).  alpha_j = sum_{i >= j} U_ji t_i from the finished row.
    if (tid < N) {
        const int j = tid;
        for (int i = 1; i < N; ++i) {
            float acc = 0.f;
            for (int k = 0; k < i; ++k)
                if (k >= j) acc += sA[i * NP + k] * sA[j * NP + k];
            if (j < i) sA[j * NP + i] = -acc / sd[i];
        }
        float a = 0.f;
        for (int i = 0; i < N; ++i)
            if (i >= j) a += sA[j * NP + i] * st[i];
        sa[j] = a;
        alpha[prob * N + j] = a;
    }
    __syncthreads();                                              // (the read of sr above is behind this barrier too: sr is rewritten below)
    if (!grad) return;
    {
        const float s = wave_sum((lane < N ? sa[lane] : 0.f) + (lane + kWave < N ? sa[lane + kWave] : 0.f));
        if (tid == 0 && dmean) dmean[prob] = wc * s;
    }
    // K^-1 = U U^T over the lower triangle (L is done with); its diagonal in sr (the diagonal of sA is U's, still read here)
    for (int idx = tid; idx < NN; idx += kT) {
        int i = idx / N, j = idx - i * N;
        if (j <= i) {
            float acc = 0.f;
            for (int k = i; k < N; ++k) acc += sA[i * NP + k] * sA[j * NP + k];
            if (j == i) sr[i] = acc;
            else sA[i * NP + j] = acc;
        }
    }
    __syncthreads();
    // G = 1/2 (alpha alpha^T - K^-1);  out = cls_weight_c sv_c G;  dsv = cls_weight_c <G, E>
    const float os = wc * sc;
    float dot = 0.f;
    for (int idx = tid; idx < NN; idx += kT) {
        int i = idx / N, j = idx - i * N;
        const float kinv = i == j ? sr[i] : (j < i ? sA[i * NP + j] : sA[j * NP + i]);
        const float gij = 0.5f * (sa[i] * sa[j] - kinv);
        Gp[idx] = os * gij;
        dot += gij * Ep[idx];
    }
    dot = wave_sum(dot);
    if (lane == 0) sred[wave] = dot;
    __syncthreads();
    if (tid == 0 && dsv) dsv[prob] = wc * ((sred[0] + sred[1]) + (sred[2] + sred[3]));
}

// a lane per (query, class): W lanes per query (W a power of two >= C, the lanes c >= C idle), kT / W queries per workgroup
__global__ __launch_bounds__(kT) void dirichlet_proba_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                            const float* __restrict__ eps, float* __restrict__ prob,
                                                            int32_t* __restrict__ labels, long BM, int C, int M, int S, int W) {
    const int tid = threadIdx.x;
    const int c = tid & (W - 1);
    const long gq = (long)blockIdx.x * (kT / W) + tid / W;          // b * M + q
    const bool live = gq < BM && c < C;
    float m = 0.f, sd = 0.f;
    if (live) {
        const long b = gq / M, q = gq - b * M;
        const long at = (b * C + c) * M + q;
        m = mu[at];
        sd = sqrtf(fmaxf(var[at], 0.f));
    }
    float acc = 0.f, lost = 0.f;                                    // compensated: S terms of up to 1 each, and the rows have to sum to 1
    for (int s = 0; s < S; ++s) {
        const float f = live ? m + sd * eps[(long)s * C + c] : -INFINITY;
        float top = f;
        for (int o = W >> 1; o > 0; o >>= 1) top = fmaxf(top, __shfl_xor(top, o, kWave));
        const float e = live ? expf(f - top) : 0.f;
        float z = e;
        for (int o = W >> 1; o > 0; o >>= 1) z += __shfl_xor(z, o, kWave);
        const float term = e / z - lost, next = acc + term;
        lost = (next - acc) - term;
        acc = next;
    }
    // argmax_c mu, the first maximum wins
    float best = live ? m : -INFINITY;
    int at = live ? c : 0x7fffffff;
    for (int o = W >> 1; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, kWave);
        const int oa = __shfl_xor(at, o, kWave);
        if (ob > best || (ob == best && oa < at)) {
            best = ob;
            at = oa;
        }
    }
    if (live) {
        prob[gq * C + c] = acc / (float)S;
        if (labels && c == 0) labels[gq] = at;
    }
}

}  // namespace

extern "C" size_t dkt_mll_rownoise_workspace_bytes(int B, int C, int N) {
    if (B <= 0 || C <= 0 || N <= 0) return 0;
    return (size_t)B * C * N * N * sizeof(float);
}

extern "C" int dkt_mll_rownoise_f32(const float* E, long e_batch_stride, long e_class_stride, const float* Y, long y_batch_stride,
                                    const float* noise_rows, long nr_batch_stride, const float* sv, const float* mean,
                                    const float* cls_weight, float* logp, float* alpha, float* dE, float* dsv, float* dmean, float* chol,
                                    int* info, int B, int C, int N, unsigned flags, void* workspace, size_t workspace_bytes, void* stream) {
    if (!E || !Y || !noise_rows || !sv || !mean || !logp || !alpha || !info || B <= 0 || C <= 0 || N <= 0) return DKT_ERR_BAD_ARG;
    if (e_batch_stride < 0 || e_class_stride < 0 || y_batch_stride < 0 || nr_batch_stride < 0) return DKT_ERR_BAD_ARG;
    if (flags & ~(DKT_MLL_WANT_GRAD | DKT_MLL_WANT_CHOL)) return DKT_ERR_BAD_ARG;
    const bool grad = flags & DKT_MLL_WANT_GRAD;
    if ((grad && !dE) || ((flags & DKT_MLL_WANT_CHOL) && !chol)) return DKT_ERR_BAD_ARG;
    if (N > DKT_LAPLACE_MAX_N || C > DKT_LAPLACE_MAX_C) return DKT_ERR_SHAPE;
    if ((long long)B * C > 0x7fffffffLL || (long long)B * N * N > 0x7fffffffLL * (long long)kT) return DKT_ERR_TOO_LARGE;
    const bool shared = grad && e_class_stride == 0;
    if (shared && (!workspace || workspace_bytes < dkt_mll_rownoise_workspace_bytes(B, C, N))) return DKT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = rownoise_lds_bytes(N);
    if (set_lds((const void*)rownoise_kernel, lds) != DKT_OK) return DKT_ERR_LAUNCH;
    float* g_out = shared ? (float*)workspace : dE;
    hipLaunchKernelGGL(rownoise_kernel, dim3((unsigned)(B * C)), dim3(kT), lds, st, E, e_batch_stride, e_class_stride, Y, y_batch_stride,
                       noise_rows, nr_batch_stride, sv, mean, cls_weight, logp, alpha, g_out, dE, dsv, dmean, chol, info, B, C, N, flags, 0);
    if (hipGetLastError() != hipSuccess) return DKT_ERR_LAUNCH;
    if (shared) {
        const long long total = (long long)B * N * N;
        hipLaunchKernelGGL(rownoise_kernel, dim3((unsigned)((total + kT - 1) / kT)), dim3(kT), 0, st, E, e_batch_stride, e_class_stride, Y,
                           y_batch_stride, noise_rows, nr_batch_stride, sv, mean, cls_weight, logp, alpha, g_out, dE, dsv, dmean, chol, info,
                           B, C, N, flags, 1);
        if (hipGetLastError() != hipSuccess) return DKT_ERR_LAUNCH;
    }
    return DKT_OK;
}

extern "C" int dkt_dirichlet_proba_f32(const float* mu, const float* var, const float* eps, float* prob, int32_t* labels, int B, int C,
                                       int M, int S, void* stream) {
    if (!mu || !var || !eps || !prob || B <= 0 || C <= 0 || M <= 0 || S <= 0) return DKT_ERR_BAD_ARG;
    if (C > DKT_LAPLACE_MAX_C) return DKT_ERR_SHAPE;
    int W = 1;
    while (W < C) W <<= 1;
    const long long BM = (long long)B * M, per = kT / W;
    if ((BM + per - 1) / per > 0x7fffffffLL) return DKT_ERR_TOO_LARGE;
    hipLaunchKernelGGL(dirichlet_proba_kernel, dim3((unsigned)((BM + per - 1) / per)), dim3(kT), 0, (hipStream_t)stream, mu, var, eps, prob,
                       labels, (long)BM, C, M, S, W);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}
