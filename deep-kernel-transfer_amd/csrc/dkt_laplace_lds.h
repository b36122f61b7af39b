// dkt_laplace_lds.h -- what the two Laplace kernels do alike on a problem held in LDS (dkt_gpc.hip: mode finding; dkt_laplace_grad.hip: the gradient at
// the mode): an N x N matrix in rows of N|1 floats, B = I + W^1/2 K W^1/2, its Cholesky factor over a workgroup of T threads, the terms of lml.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/dkt_abi.h"

namespace dkt_laplace {

constexpr int kWave = 64;

__host__ __device__ inline int padded(int N) { return N | 1; }          // odd row stride: a column walk touches every bank

// sum over the wave, the same value in every lane (the pairs commute: x + y in one lane, y + x in its partner)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// dst (rows of NP floats in LDS) = [sc *] src (N x N, dense), T threads
template <int T, bool SCALED = false>
__device__ __forceinline__ void stage_matrix(float* dst, const float* src, int N, int NP, int tid, float sc = 1.f) {
    for (int idx = tid; idx < N * N; idx += T) {
        int i = idx / N, j = idx - i * N;
        dst[i * NP + j] = SCALED ? sc * src[idx] : src[idx];
    }
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
// ROWS >= N rows take part: a row i >= N (a right-hand side carried along, dkt_mll_rownoise.hip) has no diagonal entry and comes out as L^-1 times it.
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

}  // namespace dkt_laplace
