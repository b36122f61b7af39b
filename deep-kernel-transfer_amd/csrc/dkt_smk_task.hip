// dkt_smk_task.hip -- libdkt_smk.so: the spectral-mixture kernel for many small tasks (include/dkt_abi_smk.h).  gfx950 only.
//
//     E[i,j] = sum_q w_q  prod_d exp(-2 pi^2 (sigma_qd tau_d)^2) cos(2 pi mu_qd tau_d),     tau = a_i - b_j
//
// Same arithmetic as csrc/dkt_spectral.hip (a mixture term as (sign, log magnitude), cos(2 pi u) as cospi(2u), the derivative of smk_bwd_kernel),
// another division of the work.  The generic kernels give one 256-thread workgroup to a matrix entry and stride its threads over D = 2916; at
// D = 40 most lanes idle and every entry pays a block reduction.  Here a workgroup holds whole tasks: their feature rows and the Q x D
// hyper-parameters sit in LDS, a lane owns whole entries and loops over d in order.  No cross-lane sum anywhere: bitwise reproducible.
//
//   smk_task_fwd_kernel  symmetric: T tasks per workgroup (T N <= 64 rows), a lane per lower-triangle entry, written to (i,j) and (j,i);
//                        cross: a workgroup per (task, 64-row chunk of x1), a lane per entry.
//   smk_task_bwd_kernel  a workgroup per task: the Q x N x N mixture terms go to LDS first, then lanes own (i, d) for dx and (q, d) for the
//                        per-task partials of dmeans / dscales (pairs i > j: both factors are even in tau), (q, i) rows for dweights.
//   smk_task_sum_kernel  the per-task partials summed over the B tasks, in a fixed order (16 contiguous runs of tasks, then the 16 run sums).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/dkt_abi.h"
#include "../../include/dkt_abi_smk.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRowStride = DKT_SMK_TASK_MAX_D + 1;   // LDS stride of a staged feature row: odd, so neighbouring lanes' rows fall on other banks
constexpr int kRows = 64;                             // x1 rows staged per forward workgroup
constexpr int kSumThreads = 1024;                     // 16 waves: 16 runs of tasks per output column
constexpr float k2Pi2 = 19.739208802178716f;          // 2 pi^2
constexpr float k4Pi2 = 39.478417604357432f;          // 4 pi^2
constexpr float k2Pi = 6.2831853071795865f;

// lower-triangle entry k (row-major, diagonal included) -> (i, j), j <= i
__device__ __forceinline__ void tri_decode(int k, int& i, int& j) {
    int r = (int)((sqrtf(8.f * (float)k + 1.f) - 1.f) * 0.5f);
    while (r * (r + 1) / 2 > k) --r;
    while ((r + 1) * (r + 2) / 2 <= k) ++r;
    i = r;
    j = k - r * (r + 1) / 2;
}

// the Q mixture terms of one entry: rows a, c (LDS), m2 = 2 mu and sg as [Q][D] (LDS), d in order
template <int Q>
__device__ __forceinline__ void mixture_terms(const float* a, const float* c, const float* m2, const float* sg, int D, float* eq) {
    float S[Q], L[Q];
    unsigned neg = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) S[q] = 0.f, L[q] = 0.f;
    for (int d = 0; d < D; ++d) {
        const float tau = a[d] - c[d];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float s = sg[q * D + d] * tau;
            S[q] = __builtin_fmaf(s, s, S[q]);
            const float cv = cospif(m2[q * D + d] * tau);
            L[q] += logf(fabsf(cv));
            neg ^= (cv < 0.f ? 1u : 0u) << q;
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float e = expf(-k2Pi2 * S[q] + L[q]);
        eq[q] = ((neg >> q) & 1u) ? -e : e;
    }
}

// LDS (dynamic, floats): xa [rows][kRowStride], xb [N][kRowStride] (cross only), m2 [Q][D], sg [Q][D], w [Q]
template <int Q, bool SYM>
__global__ __launch_bounds__(kThreads) void smk_task_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                                const float* __restrict__ wgt, const float* __restrict__ mu,
                                                                const float* __restrict__ sg, float* __restrict__ E, int B, int M,
                                                                int N, int D, int T, int chunks) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    int b0, r0, rows, nt;
    if (SYM) {
        b0 = blockIdx.x * T;
        nt = min(T, B - b0);
        rows = nt * N;
        r0 = 0;
    } else {
        b0 = blockIdx.x / chunks;
        r0 = (blockIdx.x - b0 * chunks) * kRows;
        rows = min(kRows, M - r0);
        nt = 1;
    }
    float* xa = lds;
    float* xb = xa + kRows * kRowStride;
    float* m2 = xb + (SYM ? 0 : DKT_SMK_TASK_MAX_N * kRowStride);
    float* sgs = m2 + Q * D;
    float* ws = sgs + Q * D;
    const float* src = SYM ? x1 + (size_t)b0 * N * D : x1 + ((size_t)b0 * M + r0) * D;
    for (int k = tid; k < rows * D; k += kThreads) {
        const int r = k / D;
        xa[r * kRowStride + (k - r * D)] = src[k];
    }
    if (!SYM) {
        const float* s2 = x2 + (size_t)b0 * N * D;
        for (int k = tid; k < N * D; k += kThreads) {
            const int r = k / D;
            xb[r * kRowStride + (k - r * D)] = s2[k];
        }
    }
    for (int k = tid; k < Q * D; k += kThreads) {
        m2[k] = 2.f * mu[k];
        sgs[k] = sg[k];
    }
    if (tid < Q) ws[tid] = wgt[tid];
    __syncthreads();
    const int per = SYM ? N * (N + 1) / 2 : N;
    const int count = SYM ? nt * per : rows * N;
    for (int e = tid; e < count; e += kThreads) {
        int t, i, j;
        if (SYM) {
            t = e / per;
            tri_decode(e - t * per, i, j);
        } else {
            t = 0;
            i = e / N;
            j = e - i * N;
        }
        const float* a = xa + (t * N * SYM + i) * kRowStride;
        const float* c = SYM ? xa + (t * N + j) * kRowStride : xb + j * kRowStride;
        float eq[Q];
        mixture_terms<Q>(a, c, m2, sgs, D, eq);
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) v = __builtin_fmaf(ws[q], eq[q], v);
        if (SYM) {
            float* Eb = E + (size_t)(b0 + t) * N * N;
            Eb[i * N + j] = v;
            Eb[j * N + i] = v;
        } else {
            E[((size_t)b0 * M + r0 + i) * N + j] = v;
        }
    }
}

// LDS (dynamic, floats): xs [N][kRowStride], g [N][N+1], eq [Q][N][N], mu [Q][D], m2 [Q][D], sg [Q][D], w [Q], red [Q][N]
// part [B][P], P = Q + 2 Q D: per task dweights [Q], dmeans [Q][D], dscales [Q][D]
template <int Q>
__global__ __launch_bounds__(kThreads) void smk_task_bwd_kernel(const float* __restrict__ gE, const float* __restrict__ x,
                                                                const float* __restrict__ wgt, const float* __restrict__ mu,
                                                                const float* __restrict__ sg, float* __restrict__ dx,
                                                                float* __restrict__ part, int N, int D) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int G = N + 1;
    float* xs = lds;
    float* gs = xs + N * kRowStride;
    float* eqs = gs + N * G;
    float* ms = eqs + Q * N * N;
    float* m2 = ms + Q * D;
    float* sgs = m2 + Q * D;
    float* ws = sgs + Q * D;
    float* red = ws + Q;
    const float* xb = x + (size_t)b * N * D;
    for (int k = tid; k < N * D; k += kThreads) {
        const int r = k / D;
        xs[r * kRowStride + (k - r * D)] = xb[k];
    }
    const float* gb = gE + (size_t)b * N * N;
    for (int k = tid; k < N * N; k += kThreads) {
        const int r = k / N;
        gs[r * G + (k - r * N)] = gb[k];
    }
    for (int k = tid; k < Q * D; k += kThreads) {
        ms[k] = mu[k];
        m2[k] = 2.f * mu[k];
        sgs[k] = sg[k];
    }
    if (tid < Q) ws[tid] = wgt[tid];
    __syncthreads();
    // 1. the mixture terms of the task, lower triangle mirrored
    const int per = N * (N + 1) / 2;
    for (int e = tid; e < per; e += kThreads) {
        int i, j;
        tri_decode(e, i, j);
        float eq[Q];
        mixture_terms<Q>(xs + i * kRowStride, xs + j * kRowStride, m2, sgs, D, eq);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            eqs[(q * N + i) * N + j] = eq[q];
            eqs[(q * N + j) * N + i] = eq[q];
        }
    }
    __syncthreads();
    float* pb = part + (size_t)b * (Q + 2 * Q * D);
    // 2. dweights: row sums sum_j gE[i,j] E_q[i,j], then (below) the sum over i
    for (int k = tid; k < Q * N; k += kThreads) {
        const int q = k / N, i = k - q * N;
        float s = 0.f;
        for (int j = 0; j < N; ++j) s = __builtin_fmaf(gs[i * G + j], eqs[(q * N + i) * N + j], s);
        red[k] = s;
    }
    // 3. dx: a lane per (i, d)
    //   dE_q/dtau_d = E_q (-4 pi^2 sigma^2 tau - 2 pi mu tan(2 pi mu tau)), gE[i,j] + gE[j,i] for both appearances of x_i
    for (int k = tid; k < N * D; k += kThreads) {
        const int i = k / D, d = k - i * D;
        float m[Q], s[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) m[q] = ms[q * D + d], s[q] = sgs[q * D + d];
        const float xi = xs[i * kRowStride + d];
        float acc = 0.f;
        for (int j = 0; j < N; ++j) {
            if (j == i) continue;
            const float g12 = gs[i * G + j] + gs[j * G + i];
            const float tau = xi - xs[j * kRowStride + d];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float cw = ws[q] * eqs[(q * N + i) * N + j];
                if (cw == 0.f) continue;                // the term underflowed (uniform over the lanes of one row i)
                float sn, cs;
                sincospif(2.f * m[q] * tau, &sn, &cs);
                if (fabsf(cs) < 1e-30f) cs = copysignf(1e-30f, cs);
                const float t = sn / cs;
                const float st = s[q] * tau;
                acc = __builtin_fmaf(g12 * cw, -k4Pi2 * s[q] * st - k2Pi * m[q] * t, acc);
            }
        }
        dx[((size_t)b * N + i) * D + d] = acc;
    }
    // 4. dmeans / dscales partials: a lane per (q, d), pairs i > j taken once with gE[i,j] + gE[j,i] (tau tan(2 pi mu tau) and tau^2 are even in tau)
    //   dE_q/dmu_d = E_q (-2 pi tau tan(2 pi mu tau)),  dE_q/dsigma_d = E_q (-4 pi^2 sigma tau^2)
    for (int k = tid; k < Q * D; k += kThreads) {
        const int q = k / D, d = k - q * D;
        const float m = ms[k], s = sgs[k], w = ws[q];
        float am = 0.f, as = 0.f;
        for (int i = 1; i < N; ++i) {
            const float xi = xs[i * kRowStride + d];
            for (int j = 0; j < i; ++j) {
                const float cw = w * eqs[(q * N + i) * N + j];
                if (cw == 0.f) continue;                // uniform over the lanes of one q
                const float g = (gs[i * G + j] + gs[j * G + i]) * cw;
                const float tau = xi - xs[j * kRowStride + d];
                float sn, cs;
                sincospif(2.f * m * tau, &sn, &cs);
                if (fabsf(cs) < 1e-30f) cs = copysignf(1e-30f, cs);
                const float t = sn / cs;
                const float st = s * tau;
                am = __builtin_fmaf(g, -k2Pi * tau * t, am);
                as = __builtin_fmaf(g, -k4Pi2 * st * tau, as);
            }
        }
        pb[Q + k] = am;
        pb[Q + Q * D + k] = as;
    }
    __syncthreads();
    if (tid < Q) {
        float s = 0.f;
        for (int i = 0; i < N; ++i) s += red[tid * N + i];
        pb[tid] = s;
    }
}

// out[p] = sum_b part[b][p]: wave w sums the tasks [w c, (w + 1) c) in order, c = ceil(B / 16), then wave 0 the 16 run sums in order
__global__ __launch_bounds__(kSumThreads) void smk_task_sum_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                   float* __restrict__ dmu, float* __restrict__ dsg, int B, int Q, int QD) {
    __shared__ float red[kSumThreads / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = Q + 2 * QD;
    const int p = blockIdx.x * 64 + lane;
    const int c = (B + kSumThreads / 64 - 1) / (kSumThreads / 64);
    const int b0 = wave * c, b1 = min(B, b0 + c);
    float s = 0.f;
    if (p < P)
        for (int b = b0; b < b1; ++b) s += part[(size_t)b * P + p];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && p < P) {
        float t = red[0][lane];
#pragma unroll
        for (int w = 1; w < kSumThreads / 64; ++w) t += red[w][lane];
        if (p < Q)
            dw[p] = t;
        else if (p < Q + QD)
            dmu[p - Q] = t;
        else
            dsg[p - Q - QD] = t;
    }
}

size_t fwd_lds_bytes(int Q, int D, bool sym) {
    return ((size_t)kRows * kRowStride + (sym ? 0 : (size_t)DKT_SMK_TASK_MAX_N * kRowStride) + 2 * (size_t)Q * D + Q) * sizeof(float);
}

size_t bwd_lds_bytes(int N, int D, int Q) {
    return ((size_t)N * kRowStride + (size_t)N * (N + 1) + (size_t)Q * N * N + 3 * (size_t)Q * D + Q + (size_t)Q * N) * sizeof(float);
}

template <int Q>
int fwd_launch(const float* x1, const float* x2, const float* w, const float* mu, const float* sg, float* E, int B, int M, int N, int D,
               hipStream_t st) {
    if (!x2) {
        const int per = N * (N + 1) / 2;
        const int T = max(1, min(kRows / N, (kThreads + per - 1) / per));
        hipLaunchKernelGGL((smk_task_fwd_kernel<Q, true>), dim3((B + T - 1) / T), dim3(kThreads), fwd_lds_bytes(Q, D, true), st, x1, x2, w,
                           mu, sg, E, B, M, N, D, T, 1);
    } else {
        const int chunks = (M + kRows - 1) / kRows;
        hipLaunchKernelGGL((smk_task_fwd_kernel<Q, false>), dim3((unsigned)B * chunks), dim3(kThreads), fwd_lds_bytes(Q, D, false), st, x1,
                           x2, w, mu, sg, E, B, M, N, D, 1, chunks);
    }
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}

template <int Q>
int bwd_launch(const float* gE, const float* x, const float* w, const float* mu, const float* sg, float* dx, float* dw, float* dmu, float* dsg,
               float* part, int B, int N, int D, hipStream_t st) {
    hipLaunchKernelGGL((smk_task_bwd_kernel<Q>), dim3(B), dim3(kThreads), bwd_lds_bytes(N, D, Q), st, gE, x, w, mu, sg, dx, part, N, D);
    if (hipGetLastError() != hipSuccess) return DKT_ERR_LAUNCH;
    const int P = Q + 2 * Q * D;
    hipLaunchKernelGGL(smk_task_sum_kernel, dim3((P + 63) / 64), dim3(kSumThreads), 0, st, part, dw, dmu, dsg, B, Q, Q * D);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}

}  // namespace

#define SMKT_DISPATCH(Qv, CALL)     \
    switch (Qv) {                   \
        case 1: return CALL(1);     \
        case 2: return CALL(2);     \
        case 3: return CALL(3);     \
        case 4: return CALL(4);     \
        case 5: return CALL(5);     \
        case 6: return CALL(6);     \
        case 7: return CALL(7);     \
        case 8: return CALL(8);     \
        default: return DKT_ERR_SHAPE; \
    }

extern "C" int dkt_smk_abi_version(void) { return DKT_SMK_ABI_VERSION; }

extern "C" int dkt_smk_task_f32(const float* x1, const float* x2, const float* weights, const float* means, const float* scales, float* E,
                                int B, int M, int N, int D, int Q, void* stream) {
    if (!x1 || !weights || !means || !scales || !E || B <= 0 || M <= 0 || N <= 0 || D <= 0 || Q <= 0) return DKT_ERR_BAD_ARG;
    if (!x2 && M != N) return DKT_ERR_BAD_ARG;
    if (N > DKT_SMK_TASK_MAX_N || M > (x2 ? DKT_SMK_TASK_MAX_M : DKT_SMK_TASK_MAX_N) || D > DKT_SMK_TASK_MAX_D || Q > DKT_SMK_TASK_MAX_Q)
        return DKT_ERR_SHAPE;
    if ((long long)B * ((M + kRows - 1) / kRows) > 0x7fffffffLL) return DKT_ERR_TOO_LARGE;
    hipStream_t st = (hipStream_t)stream;
#define SMKT_F(QQ) fwd_launch<QQ>(x1, x2, weights, means, scales, E, B, M, N, D, st)
    SMKT_DISPATCH(Q, SMKT_F)
#undef SMKT_F
}

extern "C" size_t dkt_smk_task_workspace_bytes(int B, int N, int D, int Q) {
    (void)N;
    if (B <= 0 || D <= 0 || Q <= 0) return 0;
    return (size_t)B * ((size_t)Q + 2 * (size_t)Q * D) * sizeof(float);
}

extern "C" int dkt_smk_task_bwd_f32(const float* gE, const float* x, const float* weights, const float* means, const float* scales, float* dx,
                                    float* dweights, float* dmeans, float* dscales, void* ws, int B, int N, int D, int Q, void* stream) {
    if (!gE || !x || !weights || !means || !scales || !dx || !dweights || !dmeans || !dscales || !ws || B <= 0 || N <= 0 || D <= 0 || Q <= 0)
        return DKT_ERR_BAD_ARG;
    if (((size_t)ws & 3) != 0) return DKT_ERR_BAD_ARG;
    if (N > DKT_SMK_TASK_MAX_N || D > DKT_SMK_TASK_MAX_D || Q > DKT_SMK_TASK_MAX_Q) return DKT_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
#define SMKT_B(QQ) bwd_launch<QQ>(gE, x, weights, means, scales, dx, dweights, dmeans, dscales, part, B, N, D, st)
    SMKT_DISPATCH(Q, SMKT_B)
#undef SMKT_B
}
