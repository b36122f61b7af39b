// libdkt_post.so (include/dkt_abi_post.h; docs/POSTERIOR.md): the joint posterior of B x C exact-GP regression problems at M query rows -- mean, full
// covariance, its factor, joint and marginal predictive log likelihood, function draws -- in ONE launch.
//
// ONE kernel instance, 256 threads, plain fp32 on the VALU (one sum in double, below), a workgroup per (episode, class), the problem held in LDS (dkt_lds_dense.h):
//   sweep 1   an (N + 1 + M) x (N|1) matrix: rows 0 .. N-1 the lower triangle of K, row N = y - mean, rows N+1 .. N+M = sv E_qs.  The right-looking Cholesky
//             sweep carries the extra rows through: row N -> t = L^-1 (y - mean), row N+1+q -> row q of V^T = (L^-1 sv E_qs^T)^T.
//   Sigma     mu = mean + V^T t (a thread per query row);  Sigma = sv E_qq - V^T V (+ noise I) in 4 x 4 register tiles over the lower triangle, written to
//             both triangles of `cov` (or of the workspace when cov is not asked for) from the one value: bitwise symmetric.  The N products of an
//             element of V^T V are summed in double and rounded once: where the support set explains the query rows, the latent Sigma is a small
//             remainder of terms of order sv, and a sequential fp32 sum alone costs it ten times the error of everything before (docs/POSTERIOR.md).
//   sweep 2   Sigma is staged back over the dead factor as an (M + 1) x (M|1) matrix, row M = yq - mu: the same sweep yields R and z = R^-1 (yq - mu).
//             (Sigma comes back from memory: this workgroup's own stores, behind a barrier.)  logp, lpd, chol_q and the samples are read off it.
// A pivot that is not finite and positive ends the attempt for the whole workgroup, which stages the matrix again with the next rung of the jitter ladder
// (0, jitter0, 10 jitter0, ...): decided per matrix, inside the kernel, for K and for Sigma apart.  Every sum has a fixed order that depends on nothing
// but N and M; no atomics.  Dynamic LDS is sized by the actual N and M (132100 B = 129.0 KiB at N = M = 127, the vectors included; 4080 B at the
// QMUL shape N = 5, M = 19), so small problems share a CU.
#include "../../include/dkt_abi_post.h"
#include "dkt_lds_dense.h"

namespace {

using namespace dkt_lds;                 // cholesky_lower_rows, kWave, padded, sum_le128, kHalfLog2Pi, set_lds
constexpr int kT = 256;
constexpr int kVec = 128;
constexpr int kVecs = 5;                 // sd .. sterm below

inline size_t post_lds_bytes(int N, int M) {
    const size_t first = (size_t)(N + 1 + M) * padded(N), second = (size_t)(M + 1) * padded(M);
    return ((first > second ? first : second) + kVecs * kVec) * sizeof(float);
}

struct PostArgs {
    const float *Ess, *Eqs, *Eqq, *Y, *sv, *mean, *noise, *Yq, *eps;
    float *mu, *cov, *chol, *logp, *lpd, *samples, *jit_s, *jit_q, *sigma;      // sigma: cov, or the workspace
    int32_t *info_s, *info_q;
    long ss_bs, ss_cs, qs_bs, qs_cs, qq_bs, qq_cs, ybs;
    int C, N, M, S, with_noise, max_tries;
    float jitter0;
};

// the 4 x 4 tile t of the lower triangle (tiles in row-major order of the triangle): tile row ti, tile column tj <= ti
__device__ __forceinline__ void tile_of(int t, int& ti, int& tj) {
    ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}

__global__ __launch_bounds__(kT) void posterior_kernel(PostArgs a) {
    extern __shared__ float lds[];
    const int N = a.N, M = a.M, S = a.S, NP = padded(N), MP = padded(M), MM = M * M;
    const size_t first = (size_t)(N + 1 + M) * NP, second = (size_t)(M + 1) * MP;
    float* sA = lds;                                         // sweep 1: K | y - mean | sv E_qs  ->  L | t | V^T;   sweep 2: Sigma | yq - mu  ->  R | z
    float* sd = sA + (first > second ? first : second);      // pivots of the sweep at hand
    float* smu = sd + kVec;                                  // mu
    float* sdiag = smu + kVec;                               // diag Sigma (without jitter_q)
    float* sres = sdiag + kVec;                              // yq - mu
    float* sterm = sres + kVec;                              // the terms of logp / lpd
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const long prob = blockIdx.x;
    const int b = (int)(prob / a.C), c = (int)(prob % a.C);
    const float* Ess = a.Ess + (long)b * a.ss_bs + (long)c * a.ss_cs;
    const float* Eqs = a.Eqs + (long)b * a.qs_bs + (long)c * a.qs_cs;
    const float* Eqq = a.Eqq + (long)b * a.qq_bs + (long)c * a.qq_cs;
    const float* Yp = a.Y + (long)b * a.ybs + (long)c * N;
    const float* Yq = a.Yq ? a.Yq + prob * M : nullptr;
    const float sc = a.sv[c], mean = a.mean[c], nz = a.noise[c];
    float* mu_o = a.mu ? a.mu + prob * M : nullptr;
    float* cov_o = a.cov ? a.cov + prob * MM : nullptr;
    float* chol_o = a.chol ? a.chol + prob * MM : nullptr;
    float* smp_o = a.samples ? a.samples + prob * (long)S * M : nullptr;
    float* sig = a.sigma + prob * MM;                        // Sigma of this problem: cov_o, or its slice of the workspace
    const float nan = __builtin_nanf("");

    // ---- sweep 1 under the jitter ladder: K, y - mean and sv E_qs in, L, t and V^T out
    int bad = 0;
    float jit = 0.f;
    for (int attempt = 0; attempt <= a.max_tries; ++attempt) {
        jit = dkt_jitter_rung(a.jitter0, attempt);
        __syncthreads();                                     // (the reads of the attempt before)
        const float dg = nz + jit;
        stage_lower_rhs<kT>(sA, Ess, sc, [=](int) { return dg; }, [=](int i) { return Yp[i] - mean; }, N, NP, tid);
        for (int idx = tid; idx < M * N; idx += kT) {
            const int q = idx / N, k = idx - q * N;
            sA[(N + 1 + q) * NP + k] = sc * Eqs[idx];
        }
        __syncthreads();
        bad = cholesky_lower_rows<kT, true>(sA, sd, N, N + 1 + M, NP, tid);
        if (!bad) break;
    }
    if (tid == 0) {
        a.info_s[prob] = bad;
        a.jit_s[prob] = jit;
    }
    if (bad) {                                               // every rung failed: NaN everywhere; info_q, jitter_q as the ladder over a NaN Sigma leaves them
        if (tid == 0) {
            a.info_q[prob] = 1;
            a.jit_q[prob] = dkt_jitter_rung(a.jitter0, a.max_tries);
            if (a.logp) a.logp[prob] = nan;
            if (a.lpd) a.lpd[prob] = nan;
        }
        if (mu_o && tid < M) mu_o[tid] = nan;
        for (int idx = tid; idx < MM; idx += kT) {
            if (cov_o) cov_o[idx] = nan;
            if (chol_o) chol_o[idx] = nan;
        }
        if (smp_o)
            for (int idx = tid; idx < S * M; idx += kT) smp_o[idx] = nan;
        return;
    }

    // ---- mu = mean + V^T t: a thread per query row (lanes NP words apart: every bank once)
    if (tid < M) {
        const float* v = sA + (N + 1 + tid) * NP;
        const float* t = sA + N * NP;
        float acc = 0.f;
        for (int k = 0; k < N; ++k) acc += v[k] * t[k];
        const float m = mean + acc;
        smu[tid] = m;
        if (mu_o) mu_o[tid] = m;
        sres[tid] = Yq ? Yq[tid] - m : 0.f;
    }
    // ---- Sigma = sv E_qq - V^T V (+ noise I) over the lower triangle in 4 x 4 tiles, both triangles from the one value
    {
        const float nq = a.with_noise ? nz : 0.f;
        const int nt = (M + 3) >> 2, ntl = nt * (nt + 1) / 2;
        for (int t = tid; t < ntl; t += kT) {
            int ti, tj;
            tile_of(t, ti, tj);
            const float *ra[4], *rb[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                ra[x] = sA + (N + 1 + min(4 * ti + x, M - 1)) * NP;      // (rows past M repeat row M - 1: read, never written)
                rb[x] = sA + (N + 1 + min(4 * tj + x, M - 1)) * NP;
            }
            double acc[4][4] = {};                               // (V^T V cancels against sv E_qq: summed in double, see the head of this file)
#pragma unroll 2
            for (int k = 0; k < N; ++k) {
                double av[4], bv[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    av[x] = (double)ra[x][k];
                    bv[x] = (double)rb[x][k];
                }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) acc[x][y] += av[x] * bv[y];
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const int i = 4 * ti + x, j = 4 * tj + y;
                    if (i < M && j <= i) {
                        const float s = (float)((double)(sc * Eqq[i * M + j]) - acc[x][y]) + (i == j ? nq : 0.f);
                        sig[i * M + j] = s;
                        if (j == i) sdiag[i] = s;
                        else sig[j * M + i] = s;
                    }
                }
        }
    }
    __syncthreads();                                         // V^T is done with; Sigma (this workgroup's stores), sdiag, sres, smu are in place
    // ---- lpd = sum_i log N(yq_i | mu_i, Sigma_ii)
    if (a.lpd) {
        if (tid < M) {
            const float d = sdiag[tid], r = sres[tid];
            sterm[tid] = -0.5f * logf(d) - 0.5f * r * r / d;
        }
        __syncthreads();
        const float s = sum_le128(sterm, M, lane);
        if (tid == 0) a.lpd[prob] = s - (float)M * kHalfLog2Pi;
    }

    // ---- sweep 2 under the ladder: Sigma + jitter_q I and yq - mu in, R and z = R^-1 (yq - mu) out
    for (int attempt = 0; attempt <= a.max_tries; ++attempt) {
        jit = dkt_jitter_rung(a.jitter0, attempt);
        __syncthreads();
        for (int idx = tid; idx < MM; idx += kT) {          // (not stage_lower_rhs: its source is __restrict__, and sig is what this kernel wrote)
            const int i = idx / M, j = idx - i * M;
            if (j <= i) sA[i * MP + j] = i == j ? sig[idx] + jit : sig[idx];
        }
        if (tid < M) sA[M * MP + tid] = sres[tid];
        __syncthreads();
        bad = cholesky_lower_rows<kT, true>(sA, sd, M, M + 1, MP, tid);
        if (!bad) break;
    }
    if (tid == 0) {
        a.info_q[prob] = bad;
        a.jit_q[prob] = jit;
    }
    if (bad) {                                               // mu, cov and lpd stand; what needs R is NaN
        if (tid == 0 && a.logp) a.logp[prob] = nan;
        if (chol_o)
            for (int idx = tid; idx < MM; idx += kT) chol_o[idx] = nan;
        if (smp_o)
            for (int idx = tid; idx < S * M; idx += kT) smp_o[idx] = nan;
        return;
    }
    if (tid < M) {
        const float d = sd[tid], z = sA[M * MP + tid];
        sA[tid * MP + tid] = d;                              // R's diagonal in its place (the sweep keeps the pivots apart)
        sterm[tid] = -0.5f * z * z - logf(d);
    }
    __syncthreads();
    if (a.logp) {
        const float s = sum_le128(sterm, M, lane);
        if (tid == 0) a.logp[prob] = s - (float)M * kHalfLog2Pi;
    }
    if (chol_o)
        for (int idx = tid; idx < MM; idx += kT) {
            const int i = idx / M, j = idx - i * M;
            chol_o[idx] = j <= i ? sA[i * MP + j] : 0.f;
        }
    // ---- samples[s] = mu + R eps[s]: an element per thread, the columns of R in index order
    if (smp_o) {
        const float* ep = a.eps + prob * (long)S * M;
        for (int idx = tid; idx < S * M; idx += kT) {
            const int s = idx / M, i = idx - s * M;
            const float* row = sA + i * MP;
            const float* e = ep + (long)s * M;
            float acc = 0.f;
            for (int j = 0; j <= i; ++j) acc += row[j] * e[j];
            smp_o[idx] = smu[i] + acc;
        }
    }
}

inline bool stride_ok(long cs, long size) { return cs == 0 || cs == size; }

}  // namespace

extern "C" int dkt_post_abi_version(void) { return DKT_POST_ABI_VERSION; }

extern "C" size_t dkt_posterior_workspace_bytes(int B, int C, int M, int want_cov) {
    if (want_cov || B < 1 || C < 1 || C > DKT_POST_MAX_C || M < 1 || M > DKT_POST_MAX_M) return 0;
    return (size_t)B * C * M * M * sizeof(float);
}

extern "C" int dkt_posterior_f32(const float* E_ss, long ss_bstride, long ss_cstride, const float* E_qs, long qs_bstride, long qs_cstride,
                                 const float* E_qq, long qq_bstride, long qq_cstride, const float* Y, long y_bstride, const float* sv, const float* mean,
                                 const float* noise, const float* Yq, const float* eps, int B, int C, int N, int M, int S, int with_noise, float jitter0,
                                 int max_tries, float* mu, float* cov, float* chol_q, float* logp, float* lpd, float* samples, float* jitter_s,
                                 float* jitter_q, int32_t* info_s, int32_t* info_q, void* workspace, size_t workspace_bytes, void* stream) {
    if (!E_ss || !E_qs || !E_qq || !Y || !sv || !mean || !noise || !jitter_s || !jitter_q || !info_s || !info_q || B <= 0 || max_tries < 0)
        return DKT_ERR_BAD_ARG;
    if (with_noise != 0 && with_noise != 1) return DKT_ERR_BAD_ARG;
    if ((logp || lpd) && !Yq) return DKT_ERR_BAD_ARG;
    if (S > 0 ? (!eps || !samples) : (eps || samples)) return DKT_ERR_BAD_ARG;
    if (N < 1 || N > DKT_POST_MAX_N || M < 1 || M > DKT_POST_MAX_M || C < 1 || C > DKT_POST_MAX_C || S < 0) return DKT_ERR_SHAPE;
    if (ss_bstride < 0 || qs_bstride < 0 || qq_bstride < 0 || y_bstride < 0 || !stride_ok(ss_cstride, (long)N * N) ||
        !stride_ok(qs_cstride, (long)M * N) || !stride_ok(qq_cstride, (long)M * M))
        return DKT_ERR_BAD_ARG;
    if ((long long)B * C > 0x7fffffffLL || (long long)S * M > 0x7fffffffLL) return DKT_ERR_TOO_LARGE;
    const size_t need = dkt_posterior_workspace_bytes(B, C, M, cov != nullptr);
    if (need && (!workspace || workspace_bytes < need)) return DKT_ERR_WORKSPACE;
    const size_t lds = post_lds_bytes(N, M);
    if (set_lds((const void*)posterior_kernel, lds) != DKT_OK) return DKT_ERR_LAUNCH;
    const PostArgs a = {E_ss, E_qs, E_qq, Y, sv, mean, noise, Yq, eps, mu, cov, chol_q, logp, lpd, samples, jitter_s, jitter_q,
                        cov ? cov : (float*)workspace, info_s, info_q, ss_bstride, ss_cstride, qs_bstride, qs_cstride, qq_bstride, qq_cstride,
                        y_bstride, C, N, M, S, with_noise, max_tries, jitter0};
    hipLaunchKernelGGL(posterior_kernel, dim3((unsigned)((long long)B * C)), dim3(kT), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}
