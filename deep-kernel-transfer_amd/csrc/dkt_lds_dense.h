// dkt_lds_dense.h -- what the kernels that keep ONE small dense problem in LDS do alike, over a workgroup of T threads in plain fp32: an N x N matrix in rows
// of N|1 floats.  Two groups of users:
//   the Laplace kernels (dkt_gpc.hip: mode finding; dkt_laplace_grad.hip: the gradient at the mode): B = I + W^1/2 K W^1/2, its Cholesky factor, the terms of lml;
//   the factor-and-invert family (dkt_mll_rownoise.hip, N x N and feature space; csrc_ext/dkt_loo.hip; dkt_laplace_grad.hip): the inverse inside the factor's own
//   storage, in this order --
//     stage_lower_rhs       the lower triangle of the matrix, a right-hand side as row N;
//     cholesky_lower_rows   L over the strict lower triangle, the pivots apart in sd, row N -> t = L^-1 rhs;
//     seed_upper_diagonal + upper_inverse_rows   U = L^-T into the upper triangle, which the factor leaves free;
//     upper_row_dot         alpha = U t;
//     gram_of_upper         the inverse U U^T back over the lower triangle (L is done with), its diagonal apart in sr (the diagonal of sA is U's, still read);
//     sym_at                reads the symmetric inverse from the lower triangle + sr.
// The LDS layout, the outputs and the NaN owners are each kernel's own.  Every sum here has a fixed order that depends on nothing but N.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/dkt_abi.h"

// Rung `attempt` of the jitter ladder 0, jitter0, 10 jitter0, 100 jitter0, ... (by repeated multiplication: the bits every ladder of the project reports in
// jitter_used).  Here, not in dkt_common.h (which includes this header): csrc_ext/dkt_loo.hip climbs the same ladder without dkt_common.h.
__host__ __device__ inline float dkt_jitter_rung(float jitter0, int attempt) {
    float jit = 0.f;
    if (attempt > 0) {
        jit = jitter0;
        for (int i = 1; i < attempt; ++i) jit *= 10.f;
    }
    return jit;
}

namespace dkt_lds {

constexpr int kWave = 64;
constexpr float kHalfLog2Pi = 0.918938533204672742f;                    // 1/2 log 2 pi (= DKT_HALF_LOG_2PI: dkt_mll.h checks)

__host__ __device__ inline int padded(int N) { return N | 1; }          // odd row stride: a column walk touches every bank

// sum over the wave, the same value in every lane (the pairs commute: x + y in one lane, y + x in its partner)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// the sum of the N <= 128 words of s, the same bits in every lane of every wave: word `lane` + word `lane + 64`, then the wave
__device__ __forceinline__ float sum_le128(const float* s, int N, int lane) {
    return wave_sum((lane < N ? s[lane] : 0.f) + (lane + kWave < N ? s[lane + kWave] : 0.f));
}

// the cross-wave tail of a sum over 256 threads: the four waves' partials, in pairs
__device__ __forceinline__ float block_sum4(const float* sred) { return (sred[0] + sred[1]) + (sred[2] + sred[3]); }

// dE[b] = sum_c G[b, c] (matrices of NN floats), the classes in index order: an element per thread of a grid of T-thread workgroups
template <int T>
__device__ __forceinline__ void sum_classes(const float* G, float* dE, int B, int C, int NN) {
    const long e = (long)blockIdx.x * T + threadIdx.x;
    if (e < (long)B * NN) {
        const long b = e / NN, r = e - b * NN;
        const float* src = G + b * C * (long)NN + r;
        float acc = src[0];
        for (int c = 1; c < C; ++c) acc += src[(long)c * NN];
        dE[e] = acc;
    }
}

// dst (rows of NP floats in LDS) = [sc *] src (N x N, dense), T threads
template <int T, bool SCALED = false>
__device__ __forceinline__ void stage_matrix(float* dst, const float* src, int N, int NP, int tid, float sc = 1.f) {
    for (int idx = tid; idx < N * N; idx += T) {
        int i = idx / N, j = idx - i * N;
        dst[i * NP + j] = SCALED ? sc * src[idx] : src[idx];
    }
}

// the lower triangle of sc E + diag(diag(i)), and row N = rhs(i)
template <int T, class Diag, class Rhs>
__device__ __forceinline__ void stage_lower_rhs(float* sA, const float* __restrict__ E, float sc, Diag diag, Rhs rhs, int N, int NP, int tid) {
    for (int idx = tid; idx < N * N; idx += T) {
        int i = idx / N, j = idx - i * N;
        if (j <= i) sA[i * NP + j] = sc * E[idx] + (i == j ? diag(i) : 0.f);
    }
    if (tid < N) sA[N * NP + tid] = rhs(tid);
}

// B = I + W^1/2 K W^1/2, lower triangle
template <int T>
__device__ __forceinline__ void build_b_lower(float* sA, const float* sK, const float* sw, int N, int NP, int tid) {
    for (int idx = tid; idx < N * N; idx += T) {
        int i = idx / N, j = idx - i * N;
        if (j <= i) sA[i * NP + j] = (i == j ? 1.f : 0.f) + (sw[i] * sK[i * NP + j]) * sw[j];
    }
}

// right-looking Cholesky: column j scaled by its pivot (kept apart in sd: the pivot entry itself is only read here), then the trailing update; two
// barriers per column.  L is the strict lower triangle of sA with sd as its diagonal; the upper triangle is not touched.
// ROWS >= N rows take part: a row i >= N (a right-hand side carried along, stage_lower_rhs) has no diagonal entry and comes out as L^-1 times it.
// CHECK: a pivot that is not finite and positive ends the sweep; returns 1 + its index, else 0 (every thread reads the same pivot, so the whole
// workgroup leaves together).
template <int T, bool CHECK>
__device__ __forceinline__ int cholesky_lower_rows(float* sA, float* sd, int N, int rows, int NP, int tid) {
    for (int j = 0; j < N; ++j) {
        const float p = sA[j * NP + j];
        if (CHECK && !(p > 0.f && p < INFINITY)) return j + 1;
        float d = sqrtf(p);
        for (int i = j + 1 + tid; i < rows; i += T) sA[i * NP + j] = sA[i * NP + j] / d;
        if (tid == 0) sd[j] = d;
        __syncthreads();
        for (int i = j + 1 + tid / 16; i < rows; i += T / 16) {
            float lij = sA[i * NP + j];
            const int kend = i < N ? i : N - 1;
            for (int k = j + 1 + (tid & 15); k <= kend; k += 16) sA[i * NP + k] -= lij * sA[k * NP + j];
        }
        __syncthreads();
    }
    return 0;
}

template <int T>
__device__ __forceinline__ void cholesky_lower(float* sA, float* sd, int N, int NP, int tid) {
    cholesky_lower_rows<T, false>(sA, sd, N, N, NP, tid);
}

// U_jj = 1 / L_jj, by the thread j < N that owns row j of U (a barrier before upper_inverse_rows)
__device__ __forceinline__ void seed_upper_diagonal(float* sA, const float* sd, int j, int NP) { sA[j * NP + j] = 1.f / sd[j]; }

// U = L^-T into the upper triangle, row i of L^-1 at a time: U_ji = -(sum_{k=j}^{i-1} L_ik U_jk) / L_ii, j < i.  Thread j < N owns row j of U (N <= the
// workgroup): it reads its own earlier writes and the rows of L, which nobody writes -- no barrier inside, and the finished row may be read by its owner at once
// (upper_row_dot).  The k loop is the same for every lane (guarded, not started at the lane's own j): at a given k the lanes read sA[j * NP + k], NP words apart
// (odd: every bank once), where a loop from k = j would walk the diagonal, NP + 1 apart -- one bank for the whole wave at NP = 127, 63, 31.  Same terms in the
// same order per element.
__device__ __forceinline__ void upper_inverse_rows(float* sA, const float* sd, int N, int NP, int tid) {
    if (tid < N) {
        const int j = tid;
        for (int i = 1; i < N; ++i) {
            float acc = 0.f;
            for (int k = 0; k < i; ++k)
                if (k >= j) acc += sA[i * NP + k] * sA[j * NP + k];
            if (j < i) sA[j * NP + i] = -acc / sd[i];
        }
    }
}

// sum_{i >= j} U_ji v_i: element j of U v (alpha = U t), by the owner of row j, guarded like the loop above
__device__ __forceinline__ float upper_row_dot(const float* sA, const float* v, int j, int N, int NP) {
    float a = 0.f;
    for (int i = 0; i < N; ++i)
        if (i >= j) a += sA[j * NP + i] * v[i];
    return a;
}

struct unscaled {
    __device__ __forceinline__ float operator()(int, int, float acc) const { return acc; }
};

// scale(i, j, (U U^T)_ij) over the lower triangle, its diagonal into sr: the inverse of what was factored, L U = I
template <int T, class Scale = unscaled>
__device__ __forceinline__ void gram_of_upper(float* sA, float* sr, int N, int NP, int tid, Scale scale = Scale()) {
    for (int idx = tid; idx < N * N; idx += T) {
        int i = idx / N, j = idx - i * N;
        if (j <= i) {
            float acc = 0.f;
            for (int k = i; k < N; ++k) acc += sA[i * NP + k] * sA[j * NP + k];
            acc = scale(i, j, acc);
            if (j == i) sr[i] = acc;
            else sA[i * NP + j] = acc;
        }
    }
}

// element (i, j) of the symmetric matrix gram_of_upper left: the strict lower triangle of sA, the diagonal in sr
__device__ __forceinline__ float sym_at(const float* sA, const float* sr, int i, int j, int NP) {
    return i == j ? sr[i] : (j < i ? sA[i * NP + j] : sA[j * NP + i]);
}

// row i of lml = -1/2 a.f - sum log(1 + exp(-(2y - 1) f)) - sum log L_ii    (log(1 + exp(-z)) = max(-z, 0) + log1p(exp(-|z|)): no overflow for large |f|)
__device__ __forceinline__ float lml_term(float y, float a, float f, float d) {
    const float z = (2.f * y - 1.f) * f;
    return -0.5f * a * f - (fmaxf(-z, 0.f) + log1pf(expf(-fabsf(z)))) - logf(d);
}

// dynamic LDS beyond 64 KiB has to be asked for
inline int set_lds(const void* fn, size_t bytes) {
    if (bytes <= 64 * 1024) return DKT_OK;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}

}  // namespace dkt_lds
