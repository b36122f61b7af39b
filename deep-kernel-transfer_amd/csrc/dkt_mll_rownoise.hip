// dkt_mll_rownoise_f32 / dkt_dirichlet_proba_f32 (include/dkt_abi.h; docs/DIRICHLET.md): the exact-GP marginal likelihood of B x C problems
// K = sv_c E + diag(noise_rows_c) -- a noise per ROW, what a Dirichlet classification likelihood makes of the class labels -- and the class
// probabilities of its latent posterior.
//
// TWO kernel instances, 256 threads each, plain fp32 on the VALU (the choice against the fp32 MFMA route of dkt_mll_mfma.hip: docs/DIRICHLET.md).
// rownoise_kernel, pass 0: a workgroup per (episode, class).  ONE (N + 1) x (N|1) matrix in LDS (64 KiB + 2.5 KiB of vectors at N = 127: two workgroups
// per CU).  Rows 0 .. N-1 hold the lower triangle of K, row N holds r = y - mean: the right-looking Cholesky sweep that turns the rows into L turns row N
// into t = L^-1 r, the forward substitution, at no barrier of its own.  logp = -1/2 t.t - sum log L_ii - N/2 log 2 pi.  Then the inverse
// inside the factor's own storage (the family of dkt_lds_dense.h, explained there): U = L^-T row by row into the upper triangle, alpha = U t, K^-1 = U U^T
// back over the lower triangle (its diagonal apart), G = 1/2 (alpha alpha^T - K^-1) written straight from it.  No jitter ladder: a pivot that is not finite and
// positive ends the problem (info, NaN outputs).  A shared E (class stride 0) has its classes summed by pass 1 of the SAME kernel (an element per
// thread, the classes in index order) from the per-class matrices pass 0 left in the workspace: no atomics, and the sum of a shared call is bit for
// bit the sum of the per-class call's outputs.  Every reduction has a fixed order that depends on nothing but N.
// dirichlet_proba_kernel: a group of W = 2^ceil(log2 C) lanes per query, a lane per class; max and sum over the classes by xor butterflies inside
// the group, the samples in index order (a compensated sum).  Its passes 1 .. 3 are the feature-space calls dkt_rownoise_lowrank_* (below).
#include "dkt_lds_dense.h"

namespace {

using namespace dkt_lds;                 // the factor-and-invert family of dkt_lds_dense.h, kWave, padded, wave_sum, kHalfLog2Pi, set_lds
constexpr int kT = 256;
constexpr int kVec = 128;
constexpr int kVecs = 5;                 // sd .. sred below

inline size_t rownoise_lds_bytes(int N) { return ((size_t)(N + 1) * padded(N) + kVecs * kVec) * sizeof(float); }

// ---- the feature-space passes (dkt_rownoise_lowrank_*; docs/DIRICHLET.md "Above 127 rows") -------------------------------------------------
// Passes 1 .. 3 of dirichlet_proba_kernel (a runtime argument; pass 0 is the class probabilities), NOT of rownoise_kernel: with them inside, that
// kernel's N x N pass measured 0.9 % (1024 x 5 x 105) and 6 % (1024 x 5 x 25) slower than before, with its own code unchanged (the runs: docs/DIRICHLET.md
// "The resident call against the parent commit"); it stays as it was.
// K = s Z Z^T + Lambda is never formed: B = I + s Z^T Lambda^-1 Z (kDP x kDP, eigenvalues >= 1) takes the place of K in the SAME LDS layout -- rows
// 0 .. kDP-1 its lower triangle, row kDP the right-hand side u = Z^T Lambda^-1 r -- and goes through the same sweep, the same U = L^-T and B^-1 = U U^T.
// The state of a problem (b, c): t = B^-1 u [kDP], then B^-1 [kDP, kDP] (symmetric, both triangles), zero-padded features included (B^-1 = I there).
constexpr int kDP = DKT_LOWRANK_DP;      // features, zero-padded to it
constexpr int kDPP = kDP | 1;            // row stride of B in LDS (= padded(kDP))
constexpr int kRows = 64;                // rows of Z a workgroup holds at a time
constexpr int kQueries = 32;             // queries of Zq a workgroup holds
constexpr int kZ4 = kDP + 4;             // row stride of a chunk of Z read by float4 along a row
constexpr int kZ1 = kDP + 1;             // ... read by scalars down a column
constexpr int kState = kDP * (kDP + 1);  // floats per problem
static_assert(kDP == 64 && kRows == 64 && kT == 256, "the 4 x 4 register tiles below cover 64 x 64 with 256 threads");

inline size_t lowrank_fwd_lds_bytes() { return ((size_t)kRows * kZ4 + 2 * kRows + (kDP + 1) * kDPP + kVecs * kVec) * sizeof(float); }
inline size_t lowrank_bwd_lds_bytes() { return ((size_t)kDP * kDP + 3 * kRows + kRows * kZ1) * sizeof(float); }
inline size_t lowrank_predict_lds_bytes() { return ((size_t)kDP * kDP + kDP + kQueries * kZ1) * sizeof(float); }

// the arguments of a feature-space pass (dirichlet_proba_kernel carries them: pass 0 is the class probabilities)
struct LowrankArgs {
    const float *Z, *Y, *NR, *sv, *mean, *cw, *gobj;
    float *o0, *o1, *dz, *dsv, *dmean, *state;
    int* io;
    long ybs, nbs;
    int C, N, D, pass;
};

// rows i0 .. i0 + ROWS - 1 of Z [N, D] -> dst (rows of `stride` floats), rows past N and features past D zero
template <int ROWS>
__device__ __forceinline__ void stage_rows(float* dst, int stride, const float* __restrict__ Zp, int i0, int N, int D, int tid) {
    const int ty = tid >> 4, c4 = (tid & 15) * 4;
#pragma unroll 1
    for (int it = 0; it < ROWS / 16; ++it) {
        const int r = it * 16 + ty;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 + r < N && c4 < D) v = *reinterpret_cast<const float4*>(Zp + (long)(i0 + r) * D + c4);
        float* o = dst + r * stride + c4;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
}

// pass 1, a workgroup per (episode, class): logp, alpha, dsv, dmean, info and the state
__device__ __forceinline__ void lowrank_forward(float* lds, const float* __restrict__ Z, const float* __restrict__ Y, long ybs,
                                                const float* __restrict__ NR, long nbs, const float* __restrict__ sv,
                                                const float* __restrict__ mean, const float* __restrict__ cw, float* __restrict__ logp,
                                                float* __restrict__ alpha, float* __restrict__ dsv, float* __restrict__ dmean,
                                                float* __restrict__ state, int* __restrict__ info, int C, int N, int D) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int ty = tid >> 4, tx = tid & 15;
    float* sZ = lds;                         // a chunk of Z (16-byte aligned rows)
    float* sw = sZ + kRows * kZ4;            // 1 / noise_rows of the chunk
    float* sq = sw + kRows;                  // r / noise_rows
    float* sA = sq + kRows;                  // B (lower) + u (row kDP) -> L + L^-1 u -> U -> B^-1
    float* sd = sA + (kDP + 1) * kDPP;
    float* st = sd + kVec;                   // L^-1 u
    float* sa = st + kVec;                   // t = B^-1 u
    float* sr = sa + kVec;                   // diagonal of B^-1
    float* sred = sr + kVec;
    const long prob = blockIdx.x;
    const int b = (int)(prob / C), c = (int)(prob % C);
    const float* Zp = Z + (long)b * N * D;
    const float* Yp = Y + (long)b * ybs + (long)c * N;
    const float* Np = NR + (long)b * nbs + (long)c * N;
    const float sc = sv[c], mu = mean[c];
    const float wc = cw ? cw[c] : 1.f;
    float* Sp = state + prob * (long)kState;

    // B = I + s sum_i z_i z_i^T / lambda_i: a 4 x 4 tile per thread (both triangles: the upper one is not kept), u in wave 0; the rows in index order
    float acc[4][4] = {};
    float u = 0.f, rlr = 0.f, slog = 0.f;
    for (int i0 = 0; i0 < N; i0 += kRows) {
        stage_rows<kRows>(sZ, kZ4, Zp, i0, N, D, tid);
        if (tid < kRows) {
            float w = 0.f, q = 0.f;
            if (i0 + tid < N) {
                const float lam = Np[i0 + tid], r = Yp[i0 + tid] - mu;
                w = 1.f / lam;
                q = w * r;
                rlr += r * q;
                slog += logf(lam);
            }
            sw[tid] = w;
            sq[tid] = q;
        }
        __syncthreads();
        const int rows = min(kRows, N - i0);
#pragma unroll 1
        for (int r = 0; r < rows; ++r) {
            const float w = sw[r];
            const float4 za = *reinterpret_cast<const float4*>(sZ + r * kZ4 + 4 * ty);
            const float4 zb = *reinterpret_cast<const float4*>(sZ + r * kZ4 + 4 * tx);
            const float a[4] = {w * za.x, w * za.y, w * za.z, w * za.w};
            const float bb[4] = {zb.x, zb.y, zb.z, zb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * bb[j];
        }
        if (tid < kDP)
            for (int r = 0; r < rows; ++r) u += sZ[r * kZ4 + tid] * sq[r];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gi = 4 * ty + i, gj = 4 * tx + j;
            if (gj <= gi) sA[gi * kDPP + gj] = (gi == gj ? 1.f : 0.f) + sc * acc[i][j];
        }
    if (tid < kDP) sA[kDP * kDPP + tid] = u;
    rlr = wave_sum(rlr);                     // (wave 0 holds them; the other waves sum zeros)
    slog = wave_sum(slog);
    __syncthreads();
    const int bad = cholesky_lower_rows<kT, true>(sA, sd, kDP, kDP + 1, kDPP, tid);
    if (tid == 0) info[prob] = bad;
    if (bad) {                               // (eigenvalues >= 1: only an input that is not finite, or a noise that is not positive, gets here)
        const float nan = __builtin_nanf("");
        if (tid == 0) {
            logp[prob] = nan;
            if (dsv) dsv[prob] = nan;
            if (dmean) dmean[prob] = nan;
        }
        for (int i = tid; i < N; i += kT) alpha[prob * N + i] = nan;
        for (int idx = tid; idx < kState; idx += kT) Sp[idx] = nan;
        return;
    }
    // logp = -1/2 (r.r/lambda - s |L^-1 u|^2) - 1/2 sum log lambda - sum log L_ii - N/2 log 2 pi
    if (tid < kDP) {
        const float t = sA[kDP * kDPP + tid];
        st[tid] = t;
        sr[tid] = 0.5f * sc * t * t - logf(sd[tid]);
        seed_upper_diagonal(sA, sd, tid, kDPP);
    }
    __syncthreads();
    {
        const float lp = wave_sum(sr[lane]);         // (exactly kDP = 64 terms: no second half)
        if (tid == 0) logp[prob] = (lp - 0.5f * rlr - 0.5f * slog) - (float)N * kHalfLog2Pi;
    }
    // U = L^-T into the upper triangle, a row per thread and no barrier inside (dkt_lds_dense.h);  t = U (L^-1 u) from the finished row
    upper_inverse_rows(sA, sd, kDP, kDPP, tid);
    if (tid < kDP) {
        const float a = upper_row_dot(sA, st, tid, kDP, kDPP);
        sa[tid] = a;
        Sp[tid] = a;
    }
    __syncthreads();
    // B^-1 = U U^T over the lower triangle, its diagonal in sr
    gram_of_upper<kT>(sA, sr, kDP, kDPP, tid);
    __syncthreads();
    for (int idx = tid; idx < kDP * kDP; idx += kT) {
        const int i = idx / kDP, j = idx - i * kDP;
        Sp[kDP + idx] = i == j ? sr[i] : (j < i ? sA[i * kDPP + j] : sA[j * kDPP + i]);          // (spelled out, not sym_at: docs/MEASUREMENTS.md R18)
    }
    // d logp / d sv = 1/2 (|t|^2 - (D - tr B^-1) / s): the trace term summed as sum_i (1 - (B^-1)_ii), every term in [0, 1) and zero on the padding
    {
        const float tt = wave_sum(sa[lane] * sa[lane]), dtr = wave_sum(1.f - sr[lane]);
        if (tid == 0 && dsv) dsv[prob] = wc * (0.5f * (tt - dtr / sc));
    }
    // alpha = Lambda^-1 (r - s Z t): 16 lanes per row, a float4 of the row each, summed by xor butterflies inside the group
    float asum = 0.f;
    const float4 t4 = make_float4(sa[4 * tx], sa[4 * tx + 1], sa[4 * tx + 2], sa[4 * tx + 3]);
    for (int i0 = 0; i0 < N; i0 += kT / 16) {
        const int i = i0 + ty;
        float dot = 0.f;
        if (i < N && 4 * tx < D) {
            const float4 z = *reinterpret_cast<const float4*>(Zp + (long)i * D + 4 * tx);
            dot = (z.x * t4.x + z.y * t4.y) + (z.z * t4.z + z.w * t4.w);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) dot += __shfl_xor(dot, o, kWave);
        if (i < N && tx == 0) {
            const float a = ((Yp[i] - mu) - sc * dot) / Np[i];
            alpha[prob * N + i] = a;
            asum += a;
        }
    }
    asum = wave_sum(asum);
    if (lane == 0) sred[wave] = asum;
    __syncthreads();
    if (tid == 0 && dmean) dmean[prob] = wc * block_sum4(sred);
}

// pass 2, a workgroup per (episode, chunk of kRows rows): dZ = gobj_b sum_c cw_c s_c Lambda_c^-1 (r_c t_c^T - Z Q_c), Q_c = s_c t_c t_c^T + B_c^-1, the
// classes in index order into one 4 x 4 register tile per thread
__device__ __forceinline__ void lowrank_backward(float* lds, const float* __restrict__ Z, const float* __restrict__ Y, long ybs,
                                                 const float* __restrict__ NR, long nbs, const float* __restrict__ sv,
                                                 const float* __restrict__ mean, const float* __restrict__ cw, const float* __restrict__ state,
                                                 const float* __restrict__ gobj, float* __restrict__ dZ, int C, int N, int D) {
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    float* sQ = lds;                         // Q_c (16-byte aligned rows)
    float* st = sQ + kDP * kDP;              // t_c
    float* sco = st + kRows;                 // cw_c s_c / lambda_ci of the chunk's rows
    float* srt = sco + kRows;                // ... times r_ci
    float* sZ = srt + kRows;                 // the chunk of Z
    const int nch = (N + kRows - 1) / kRows;
    const int b = blockIdx.x / nch, i0 = (blockIdx.x % nch) * kRows;
    const float* Zp = Z + (long)b * N * D;
    stage_rows<kRows>(sZ, kZ1, Zp, i0, N, D, tid);
    float acc[4][4] = {};
    for (int c = 0; c < C; ++c) {
        const float* Sp = state + ((long)b * C + c) * kState;
        const float sc = sv[c];
        __syncthreads();                     // (the reads of the class before; the chunk of Z the first time)
#pragma unroll 1
        for (int it = 0; it < kDP * kDP / 4 / kT; ++it) {
            const int idx4 = it * kT + tid, k = idx4 >> 4, d4 = (idx4 & 15) * 4;
            const float4 bi = *reinterpret_cast<const float4*>(Sp + kDP + k * kDP + d4);
            const float4 td = *reinterpret_cast<const float4*>(Sp + d4);
            const float stk = sc * Sp[k];
            *reinterpret_cast<float4*>(sQ + k * kDP + d4) = make_float4(stk * td.x + bi.x, stk * td.y + bi.y, stk * td.z + bi.z, stk * td.w + bi.w);
        }
        if (tid < kDP) st[tid] = Sp[tid];
        if (tid < kRows) {
            float co = 0.f, rt = 0.f;
            if (i0 + tid < N) {
                co = (cw ? cw[c] : 1.f) * sc / NR[(long)b * nbs + (long)c * N + i0 + tid];
                rt = co * (Y[(long)b * ybs + (long)c * N + i0 + tid] - mean[c]);
            }
            sco[tid] = co;
            srt[tid] = rt;
        }
        __syncthreads();
        const float co[4] = {-sco[4 * ty], -sco[4 * ty + 1], -sco[4 * ty + 2], -sco[4 * ty + 3]};
#pragma unroll 1
        for (int k = 0; k < kDP; ++k) {
            const float4 q = *reinterpret_cast<const float4*>(sQ + k * kDP + 4 * tx);
            const float qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float a = co[i] * sZ[(4 * ty + i) * kZ1 + k];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += a * qq[j];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += srt[4 * ty + i] * st[4 * tx + j];
    }
    const float g = gobj[b];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = i0 + 4 * ty + i;
        if (row < N && 4 * tx < D)
            *reinterpret_cast<float4*>(dZ + ((long)b * N + row) * D + 4 * tx) = make_float4(g * acc[i][0], g * acc[i][1], g * acc[i][2], g * acc[i][3]);
    }
}

// pass 3, a workgroup per (episode, chunk of kQueries queries), 8 lanes per query (8 features each): mu = m + s z.t, var = s z^T B^-1 z, the classes in
// index order; labels = the first maximum of mu
__device__ __forceinline__ void lowrank_predict(float* lds, const float* __restrict__ Zq, const float* __restrict__ state,
                                                const float* __restrict__ sv, const float* __restrict__ mean, float* __restrict__ mu_out,
                                                float* __restrict__ var_out, int* __restrict__ labels, int C, int M, int D) {
    const int tid = threadIdx.x, q = tid >> 3, part = tid & 7;
    float* sB = lds;                         // B_c^-1 (16-byte aligned rows)
    float* st = sB + kDP * kDP;              // t_c
    float* sZ = st + kDP;                    // the chunk of queries
    const int nch = (M + kQueries - 1) / kQueries;
    const int b = blockIdx.x / nch, q0 = (blockIdx.x % nch) * kQueries;
    stage_rows<kQueries>(sZ, kZ1, Zq + (long)b * M * D, q0, M, D, tid);
    __syncthreads();
    float z[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) z[d] = sZ[q * kZ1 + part * 8 + d];
    float best = -INFINITY;
    int at = 0;
    for (int c = 0; c < C; ++c) {
        const float* Sp = state + ((long)b * C + c) * kState;
        __syncthreads();                     // (the reads of the class before)
#pragma unroll 1
        for (int it = 0; it < kDP * kDP / 4 / kT; ++it) {
            const int idx4 = it * kT + tid;
            *reinterpret_cast<float4*>(sB + idx4 * 4) = *reinterpret_cast<const float4*>(Sp + kDP + idx4 * 4);
        }
        if (tid < kDP) st[tid] = Sp[tid];
        __syncthreads();
        float m = 0.f, v = 0.f;
#pragma unroll
        for (int d = 0; d < 8; ++d) m += z[d] * st[part * 8 + d];
#pragma unroll 1
        for (int k = 0; k < kDP; ++k) {
            const float4 b0 = *reinterpret_cast<const float4*>(sB + k * kDP + part * 8);
            const float4 b1 = *reinterpret_cast<const float4*>(sB + k * kDP + part * 8 + 4);
            const float inner = ((b0.x * z[0] + b0.y * z[1]) + (b0.z * z[2] + b0.w * z[3])) + ((b1.x * z[4] + b1.y * z[5]) + (b1.z * z[6] + b1.w * z[7]));
            v += sZ[q * kZ1 + k] * inner;
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            m += __shfl_xor(m, o, kWave);
            v += __shfl_xor(v, o, kWave);
        }
        const float mu = mean[c] + sv[c] * m;
        if (mu > best) {
            best = mu;
            at = c;
        }
        if (part == 0 && q0 + q < M) {
            mu_out[((long)b * C + c) * M + q0 + q] = mu;
            var_out[((long)b * C + c) * M + q0 + q] = sv[c] * v;
        }
    }
    if (labels && part == 0 && q0 + q < M) labels[(long)b * M + q0 + q] = at;
}

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
        sum_classes<kT>(Gout, dE, B, C, NN);
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

    stage_lower_rhs<kT>(sA, Ep, sc, [=](int i) { return Np[i]; }, [=](int i) { return Yp[i] - mu; }, N, NP, tid);
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
        seed_upper_diagonal(sA, sd, tid, NP);
    }
    __syncthreads();
    {
        const float lp = sum_le128(sr, N, lane);
        if (tid == 0) logp[prob] = lp - (float)N * kHalfLog2Pi;
    }
    // U = L^-T into the upper triangle, a row per thread and no barrier inside (dkt_lds_dense.h);  alpha = U t from the finished row
    upper_inverse_rows(sA, sd, N, NP, tid);
    if (tid < N) {
        const float a = upper_row_dot(sA, st, tid, N, NP);
        sa[tid] = a;
        alpha[prob * N + tid] = a;
    }
    __syncthreads();                                              // (the read of sr above is behind this barrier too: sr is rewritten below)
    if (!grad) return;
    {
        const float s = sum_le128(sa, N, lane);
        if (tid == 0 && dmean) dmean[prob] = wc * s;
    }
    // K^-1 = U U^T over the lower triangle, its diagonal in sr
    gram_of_upper<kT>(sA, sr, N, NP, tid);
    __syncthreads();
    // G = 1/2 (alpha alpha^T - K^-1);  out = cls_weight_c sv_c G;  dsv = cls_weight_c <G, E>
    const float os = wc * sc;
    float dot = 0.f;
    for (int idx = tid; idx < NN; idx += kT) {
        int i = idx / N, j = idx - i * N;
        const float kinv = sym_at(sA, sr, i, j, NP);
        const float gij = 0.5f * (sa[i] * sa[j] - kinv);
        Gp[idx] = os * gij;
        dot += gij * Ep[idx];
    }
    dot = wave_sum(dot);
    if (lane == 0) sred[wave] = dot;
    __syncthreads();
    if (tid == 0 && dsv) dsv[prob] = wc * block_sum4(sred);
}

// a lane per (query, class): W lanes per query (W a power of two >= C, the lanes c >= C idle), kT / W queries per workgroup
__global__ __launch_bounds__(kT) void dirichlet_proba_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                            const float* __restrict__ eps, float* __restrict__ prob,
                                                            int32_t* __restrict__ labels, long BM, int C, int M, int S, int W, LowrankArgs lr) {
    // the feature-space passes (Z is the queries Zq [B,M,D] with N = M in pass 3, o0 / o1 / io are mu / var / labels there)
    if (lr.pass) {
        extern __shared__ __align__(16) float lds[];
        if (lr.pass == 1) lowrank_forward(lds, lr.Z, lr.Y, lr.ybs, lr.NR, lr.nbs, lr.sv, lr.mean, lr.cw, lr.o0, lr.o1, lr.dsv, lr.dmean, lr.state, lr.io, lr.C, lr.N, lr.D);
        else if (lr.pass == 2) lowrank_backward(lds, lr.Z, lr.Y, lr.ybs, lr.NR, lr.nbs, lr.sv, lr.mean, lr.cw, lr.state, lr.gobj, lr.dz, lr.C, lr.N, lr.D);
        else lowrank_predict(lds, lr.Z, lr.state, lr.sv, lr.mean, lr.o0, lr.o1, lr.io, lr.C, lr.N, lr.D);
        return;
    }
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
                       labels, (long)BM, C, M, S, W, LowrankArgs{});
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}

// ---- the same likelihood in feature space (linear kernels, D <= DKT_LOWRANK_DP): further passes of dirichlet_proba_kernel, no new kernel instance ----
namespace {
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int lowrank_shape(int C, int D) { return (D > kDP || D % 4 != 0 || C > DKT_LAPLACE_MAX_C) ? DKT_ERR_SHAPE : DKT_OK; }
inline int lowrank_launch(int pass, long long grid, size_t lds, hipStream_t st, const float* Z, const float* Y, long ybs, const float* NR, long nbs,
                          const float* sv, const float* mean, const float* cw, float* o0, float* o1, float* dz, float* dsv, float* dmean, int* io,
                          int B, int C, int N, float* state, const float* gobj, int D) {
    (void)B;
    if (grid > 0x7fffffffLL) return DKT_ERR_TOO_LARGE;
    if (set_lds((const void*)dirichlet_proba_kernel, lds) != DKT_OK) return DKT_ERR_LAUNCH;
    const LowrankArgs lr = {Z, Y, NR, sv, mean, cw, gobj, o0, o1, dz, dsv, dmean, state, io, ybs, nbs, C, N, D, pass};
    hipLaunchKernelGGL(dirichlet_proba_kernel, dim3((unsigned)grid), dim3(kT), lds, st, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                       (float*)nullptr, (int32_t*)nullptr, 0L, 0, 0, 0, 0, lr);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}
}  // namespace

extern "C" size_t dkt_rownoise_lowrank_state_bytes(int B, int C) {
    if (B <= 0 || C <= 0) return 0;
    return (size_t)B * C * kState * sizeof(float);
}

extern "C" int dkt_rownoise_lowrank_f32(const float* Z, const float* Y, long y_batch_stride, const float* noise_rows, long nr_batch_stride,
                                        const float* sv, const float* mean, const float* cls_weight, float* logp, float* alpha, int* info,
                                        float* dsv, float* dmean, void* state, size_t state_bytes, int B, int C, int N, int D, void* stream) {
    if (!Z || !Y || !noise_rows || !sv || !mean || !logp || !alpha || !info || !state || B <= 0 || C <= 0 || N <= 0 || D <= 0) return DKT_ERR_BAD_ARG;
    if (y_batch_stride < 0 || nr_batch_stride < 0 || !aligned16(Z) || !aligned16(state)) return DKT_ERR_BAD_ARG;
    if (lowrank_shape(C, D) != DKT_OK) return DKT_ERR_SHAPE;
    if (state_bytes < dkt_rownoise_lowrank_state_bytes(B, C)) return DKT_ERR_WORKSPACE;
    return lowrank_launch(1, (long long)B * C, lowrank_fwd_lds_bytes(), (hipStream_t)stream, Z, Y, y_batch_stride, noise_rows, nr_batch_stride, sv, mean,
                          cls_weight, logp, alpha, nullptr, dsv, dmean, info, B, C, N, (float*)state, nullptr, D);
}

extern "C" int dkt_rownoise_lowrank_bwd_f32(const float* Z, const float* Y, long y_batch_stride, const float* noise_rows, long nr_batch_stride,
                                            const float* sv, const float* mean, const float* cls_weight, const void* state, size_t state_bytes,
                                            const float* gobj, float* dZ, int B, int C, int N, int D, void* stream) {
    if (!Z || !Y || !noise_rows || !sv || !mean || !state || !gobj || !dZ || B <= 0 || C <= 0 || N <= 0 || D <= 0) return DKT_ERR_BAD_ARG;
    if (y_batch_stride < 0 || nr_batch_stride < 0 || !aligned16(Z) || !aligned16(state) || !aligned16(dZ)) return DKT_ERR_BAD_ARG;
    if (lowrank_shape(C, D) != DKT_OK) return DKT_ERR_SHAPE;
    if (state_bytes < dkt_rownoise_lowrank_state_bytes(B, C)) return DKT_ERR_WORKSPACE;
    return lowrank_launch(2, (long long)B * ((N + kRows - 1) / kRows), lowrank_bwd_lds_bytes(), (hipStream_t)stream, Z, Y, y_batch_stride, noise_rows,
                          nr_batch_stride, sv, mean, cls_weight, nullptr, nullptr, dZ, nullptr, nullptr, nullptr, B, C, N, (float*)state, gobj, D);
}

extern "C" int dkt_rownoise_lowrank_predict_f32(const float* Zq, const void* state, size_t state_bytes, const float* sv, const float* mean, float* mu,
                                                float* var, int32_t* labels, int B, int C, int M, int D, void* stream) {
    if (!Zq || !state || !sv || !mean || !mu || !var || B <= 0 || C <= 0 || M <= 0 || D <= 0) return DKT_ERR_BAD_ARG;
    if (!aligned16(Zq) || !aligned16(state)) return DKT_ERR_BAD_ARG;
    if (lowrank_shape(C, D) != DKT_OK) return DKT_ERR_SHAPE;
    if (state_bytes < dkt_rownoise_lowrank_state_bytes(B, C)) return DKT_ERR_WORKSPACE;
    return lowrank_launch(3, (long long)B * ((M + kQueries - 1) / kQueries), lowrank_predict_lds_bytes(), (hipStream_t)stream, Zq, nullptr, 0, nullptr, 0, sv,
                          mean, nullptr, mu, var, nullptr, nullptr, nullptr, labels, B, C, M, (float*)state, nullptr, D);
}
