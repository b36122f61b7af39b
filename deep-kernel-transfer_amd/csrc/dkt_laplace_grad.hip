// dkt_laplace_grad_f32 (include/dkt_abi.h): the Laplace approximation of the log marginal likelihood of B x C binary GP classifiers at their posterior
// modes, and its gradient with respect to the prior covariance (GPML algorithm 5.1 in matrix form; docs/LAPLACE.md "Training").
//
// ONE kernel instance, 256 threads.  pass 0: a workgroup per (episode, class) problem.  K_c = scale_c K and the matrix to factor stay in LDS
// (2 N (N|1) floats + 5 KiB of vectors: 131 KiB at N = 127), as in dkt_gpc.hip.  (I + W^1/2 K W^1/2)^-1 is formed inside the factor's own N x (N|1)
// storage (the family of dkt_lds_dense.h, explained there): Cholesky (strict lower triangle, the pivots apart) -> U = L^-T row by row into the UPPER triangle, which the factor leaves free -> U U^T
// back over the lower triangle (the diagonal apart), scaled to R = W^1/2 (.)^-1 W^1/2 on the way.  diag(K R K) goes one row product k_i^T R k_i at a
// time, G is written straight from R, g, u.  A shared K (class stride 0) has its classes summed by pass 1 of the SAME kernel (an element per thread,
// the classes in index order) from the per-class matrices pass 0 left in the workspace: no atomics, and the sum of a shared call is bit for bit the
// sum of the per-class call's outputs.  Plain fp32 on the VALU; every reduction has a fixed order that depends on nothing but N.
#include "dkt_lds_dense.h"

namespace {

using namespace dkt_lds;                 // padded, wave_sum, stage_matrix, build_b_lower, cholesky_lower, lml_term, set_lds and the factor-and-invert family
constexpr int kT = 256;
constexpr int kVec = 128;
constexpr int kVecs = 10;                // sf .. sred below

inline size_t grad_lds_bytes(int N) { return ((size_t)2 * N * padded(N) + kVecs * kVec) * sizeof(float); }

__global__ __launch_bounds__(kT) void laplace_grad_kernel(const float* __restrict__ K, long kbs, long kcs, const float* __restrict__ scale,
                                                         const float* __restrict__ Y, long ybs, const float* __restrict__ F,
                                                         const float* __restrict__ cw, float* __restrict__ lml_o, float* __restrict__ Gout,
                                                         float* __restrict__ dK, float* __restrict__ dscale, int B, int C, int N, int pass) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int NN = N * N;
    if (pass == 1) {
        sum_classes<kT>(Gout, dK, B, C, NN);
        return;
    }
    const int NP = padded(N);
    float* sK = lds;                     // K_c = scale_c K
    float* sA = sK + N * NP;             // B -> L (strict lower) + U = L^-T (upper, diagonal included) -> R (strict lower)
    float* sf = sA + N * NP;             // f_hat
    float* sg = sf + kVec;               // y - pi
    float* sw = sg + kVec;               // W^1/2
    float* s3 = sw + kVec;               // pi (1 - pi) (1 - 2 pi)
    float* sd = s3 + kVec;               // pivots of L
    float* sr = sd + kVec;               // diagonal of R
    float* ss = sr + kVec;               // s2
    float* st = ss + kVec;               // the terms of lml, then K s2
    float* su = st + kVec;               // u
    float* sred = su + kVec;             // cross-wave partials
    const int lane = tid & (kWave - 1), wave = tid >> 6;
    const long prob = blockIdx.x;
    const int b = (int)(prob / C), c = (int)(prob % C);
    const float* Kp = K + (long)b * kbs + (long)c * kcs;
    const float* Yp = Y + (long)b * ybs + (long)c * N;
    const float sc = scale ? scale[c] : 1.f;
    const float wc = cw ? cw[c] : 1.f;

    stage_matrix<kT, true>(sK, Kp, N, NP, tid, sc);
    if (tid < N) {
        const float f = F[prob * N + tid], y = Yp[tid];
        const float pi = 1.f / (1.f + expf(-f));
        const float w = pi * (1.f - pi);
        sf[tid] = f;
        sg[tid] = y - pi;
        sw[tid] = sqrtf(w);
        s3[tid] = w * (1.f - 2.f * pi);
    }
    __syncthreads();
    build_b_lower<kT>(sA, sK, sw, N, NP, tid);
    __syncthreads();
    cholesky_lower<kT>(sA, sd, N, NP, tid);
    // lml = -1/2 g.f - sum log(1 + exp(-(2y - 1) f)) - sum log L_ii
    if (tid < N) {
        const float f = sf[tid], g = sg[tid];
        st[tid] = lml_term(Yp[tid], g, f, sd[tid]);
        seed_upper_diagonal(sA, sd, tid, NP);
    }
    __syncthreads();
    {
        const float lml = sum_le128(st, N, lane);
        if (tid == 0) lml_o[prob] = lml;
    }
    // U = L^-T into the upper triangle, a row per thread and no barrier inside (dkt_lds_dense.h)
    upper_inverse_rows(sA, sd, N, NP, tid);
    __syncthreads();
    // (I + W^1/2 K W^1/2)^-1 = U U^T over the lower triangle, scaled to R = W^1/2 (.) W^1/2; its diagonal in sr
    gram_of_upper<kT>(sA, sr, N, NP, tid, [=](int i, int j, float acc) { return (sw[i] * acc) * sw[j]; });
    __syncthreads();
    // (from here on only the lower triangle of sA is read, as R_ij = R_ji; the U above it is dead)
    // diag(K R K)_i = k_i^T R k_i, a wave per row i, lanes over the rows j of R (j and j + 64); s2 = -1/2 (K_ii - that) pi (1 - pi) (1 - 2 pi)
    for (int i = wave; i < N; i += kT / kWave) {
        float part = 0.f;
        for (int h = 0; h < 2; ++h) {
            const int j = lane + h * kWave;
            if (j < N) {
                float v = 0.f;
                for (int k = 0; k < j; ++k) v += sA[j * NP + k] * sK[i * NP + k];
                v += sr[j] * sK[i * NP + j];
                for (int k = j + 1; k < N; ++k) v += sA[k * NP + j] * sK[i * NP + k];
                part += v * sK[i * NP + j];
            }
        }
        part = wave_sum(part);
        if (lane == 0) ss[i] = -0.5f * (sK[i * NP + i] - part) * s3[i];
    }
    __syncthreads();
    // u = s2 - R (K s2)
    if (tid < N) {
        float acc = 0.f;
        for (int j = 0; j < N; ++j) acc += sK[tid * NP + j] * ss[j];
        st[tid] = acc;
    }
    __syncthreads();
    if (tid < N) {
        const int i = tid;
        float acc = 0.f;
        for (int k = 0; k < i; ++k) acc += sA[i * NP + k] * st[k];
        acc += sr[i] * st[i];
        for (int k = i + 1; k < N; ++k) acc += sA[k * NP + i] * st[k];
        su[i] = ss[i] - acc;
    }
    __syncthreads();
    // G = 1/2 (g g^T - R) + 1/2 (u g^T + g u^T);  out = cls_weight_c scale_c G;  dscale = cls_weight_c <G, K> (the unscaled K)
    float* Gp = Gout + prob * (long)NN;
    const float os = wc * sc;
    float dot = 0.f;
    for (int idx = tid; idx < NN; idx += kT) {
        int i = idx / N, j = idx - i * N;
        const float r = sym_at(sA, sr, i, j, NP);
        const float gij = 0.5f * (sg[i] * sg[j] - r) + 0.5f * (su[i] * sg[j] + sg[i] * su[j]);
        Gp[idx] = os * gij;
        dot += gij * Kp[idx];
    }
    dot = wave_sum(dot);
    if (lane == 0) sred[wave] = dot;
    __syncthreads();
    if (tid == 0 && dscale) dscale[prob] = wc * block_sum4(sred);
}

}  // namespace

extern "C" size_t dkt_laplace_grad_workspace_bytes(int B, int C, int N) {
    if (B <= 0 || C <= 0 || N <= 0) return 0;
    return (size_t)B * C * N * N * sizeof(float);
}

extern "C" int dkt_laplace_grad_f32(const float* K, long k_batch_stride, long k_class_stride, const float* scale, const float* Y,
                                    long y_batch_stride, const float* f_hat, const float* cls_weight, float* lml, float* dK, float* dscale,
                                    int B, int C, int N, void* workspace, size_t workspace_bytes, void* stream) {
    if (!K || !Y || !f_hat || !lml || !dK || B <= 0 || C <= 0 || N <= 0) return DKT_ERR_BAD_ARG;
    if (k_batch_stride < 0 || k_class_stride < 0 || y_batch_stride < 0) return DKT_ERR_BAD_ARG;
    if (N > DKT_LAPLACE_MAX_N || C > DKT_LAPLACE_MAX_C) return DKT_ERR_SHAPE;
    if ((long long)B * C > 0x7fffffffLL || (long long)B * N * N > 0x7fffffffLL * (long long)kT) return DKT_ERR_TOO_LARGE;
    const bool shared = k_class_stride == 0;
    if (shared && (!workspace || workspace_bytes < dkt_laplace_grad_workspace_bytes(B, C, N))) return DKT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = grad_lds_bytes(N);
    if (set_lds((const void*)laplace_grad_kernel, lds) != DKT_OK) return DKT_ERR_LAUNCH;
    float* g_out = shared ? (float*)workspace : dK;
    hipLaunchKernelGGL(laplace_grad_kernel, dim3((unsigned)(B * C)), dim3(kT), lds, st, K, k_batch_stride, k_class_stride, scale, Y,
                       y_batch_stride, f_hat, cls_weight, lml, g_out, dK, dscale, B, C, N, 0);
    if (hipGetLastError() != hipSuccess) return DKT_ERR_LAUNCH;
    if (shared) {
        const long long total = (long long)B * N * N;
        hipLaunchKernelGGL(laplace_grad_kernel, dim3((unsigned)((total + kT - 1) / kT)), dim3(kT), 0, st, K, k_batch_stride, k_class_stride,
                           scale, Y, y_batch_stride, f_hat, cls_weight, lml, g_out, dK, dscale, B, C, N, 1);
        if (hipGetLastError() != hipSuccess) return DKT_ERR_LAUNCH;
    }
    return DKT_OK;
}
