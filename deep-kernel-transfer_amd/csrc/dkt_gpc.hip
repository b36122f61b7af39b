// libdkt_gpc.so (include/dkt_abi_gpc.h): Laplace-approximation GP classification at test time -- Newton mode finding (GPML algorithm 3.1) and
// prediction (algorithm 3.2 + the probit-mixture average of the sigmoid), for the one-vs-rest class models of B episodes.
//
// Mode: a workgroup per (episode, class) problem.  K and the matrix B = I + W^1/2 K W^1/2 (factored in place) live in LDS for the whole Newton
// loop, the vectors too; every iteration and the stopping test run in the kernel.  The factorisation is a right-looking Cholesky over the
// workgroup (two barriers per column), the two triangular solves run in ONE wave with the right-hand side in registers (a lane owns rows l and
// l + 64, the pivot travels by a lane read): no barrier inside them.  The C problems of an episode read a shared K from global memory once each
// (C - 1 of those reads hit L2).  Every sum has a fixed order that does not depend on the workgroup size: the results are bitwise reproducible.
//
// Predict: a wave per 64 query points of an episode, looping over the classes (the label needs all of them): the class's factor L in LDS, a
// lane solves L v = w_sr * ks for its own query (v in LDS, column per lane), var = kss - |v|^2.  The five-term mixture is summed in double:
// its coefficients are about +-2000..3500 and sum to 1, in fp32 the cancellation costs 1e-4 of the probability.
#include "../../include/dkt_abi_gpc.h"
#include "dkt_lds_dense.h"

namespace {

using namespace dkt_lds;                 // padded, sum_le128, stage_matrix, build_b_lower, cholesky_lower, lml_term, set_lds
constexpr int kVecs = 8;                 // LDS vectors of the mode kernel, 128 floats each
constexpr int kVec = 128;
constexpr int kQT = 64;                  // query points per workgroup of the predict kernel (a lane each)
constexpr int kQS = kQT + 1;             // row stride of the per-lane columns (odd: the staging writes do not collide)

inline size_t mode_lds_bytes(int N) { return ((size_t)2 * N * padded(N) + kVecs * kVec) * sizeof(float); }
inline size_t predict_lds_bytes(int N) { return ((size_t)N * padded(N) + (size_t)N * kQS + 2 * kVec) * sizeof(float); }

template <int T>
__global__ __launch_bounds__(T) void gpc_mode_kernel(const float* __restrict__ K, long kbs, long kcs, const float* __restrict__ Y, long ybs,
                                                    float* __restrict__ Fo, float* __restrict__ Go, float* __restrict__ Wo,
                                                    float* __restrict__ Lo, float* __restrict__ lml_o, int* __restrict__ it_o, int C, int N,
                                                    int max_iter) {
    extern __shared__ float lds[];
    const int NP = padded(N);
    float* sK = lds;
    float* sA = sK + N * NP;
    float* sf = sA + N * NP;             // f
    float* sy = sf + kVec;               // targets
    float* sg = sy + kVec;               // y - pi
    float* sw = sg + kVec;               // W^1/2
    float* sb = sw + kVec;               // b, then a
    float* st = sb + kVec;               // W^1/2 K b, then the terms of lml
    float* sd = st + kVec;               // diagonal of L
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const long prob = blockIdx.x;
    const int b = (int)(prob / C), c = (int)(prob % C);
    const float* Kp = K + (long)b * kbs + (long)c * kcs;
    const float* Yp = Y + (long)b * ybs + (long)c * N;

    stage_matrix<T>(sK, Kp, N, NP, tid);
    if (tid < N) {
        sy[tid] = Yp[tid];
        sf[tid] = 0.f;
    }
    __syncthreads();

    float lml_prev = -INFINITY;
    int iters = 0;
    for (int it = 0; it < max_iter; ++it) {
        // pi, W, b at the current f
        if (tid < N) {
            float f = sf[tid];
            float pi = 1.f / (1.f + expf(-f));
            float w = pi * (1.f - pi);
            float r = sy[tid] - pi;
            sg[tid] = r;
            sw[tid] = sqrtf(w);
            sb[tid] = w * f + r;
        }
        __syncthreads();
        // B = I + W^1/2 K W^1/2 (lower triangle) and t = W^1/2 K b
        build_b_lower<T>(sA, sK, sw, N, NP, tid);
        if (tid < N) {
            float acc = 0.f;
            for (int j = 0; j < N; ++j) acc += sK[tid * NP + j] * sb[j];
            st[tid] = sw[tid] * acc;
        }
        __syncthreads();
        cholesky_lower<T>(sA, sd, N, NP, tid);
        // a = b - W^1/2 L^-T L^-1 t, one wave, rows `lane` and `lane + 64` in registers
        if (tid < kWave) {
            const int i0 = lane, i1 = lane + kWave;
            float u0 = i0 < N ? st[i0] : 0.f, u1 = i1 < N ? st[i1] : 0.f;
            for (int j = 0; j < N; ++j) {
                float z = (j < kWave ? __shfl(u0, j, kWave) : __shfl(u1, j - kWave, kWave)) / sd[j];
                if (i0 == j) u0 = z;
                if (i1 == j) u1 = z;
                if (i0 > j && i0 < N) u0 -= sA[i0 * NP + j] * z;
                if (i1 > j && i1 < N) u1 -= sA[i1 * NP + j] * z;
            }
            for (int j = N - 1; j >= 0; --j) {
                float z = (j < kWave ? __shfl(u0, j, kWave) : __shfl(u1, j - kWave, kWave)) / sd[j];
                if (i0 == j) u0 = z;
                if (i1 == j) u1 = z;
                if (i0 < j) u0 -= sA[j * NP + i0] * z;
                if (i1 < j) u1 -= sA[j * NP + i1] * z;
            }
            if (i0 < N) sb[i0] = sb[i0] - sw[i0] * u0;
            if (i1 < N) sb[i1] = sb[i1] - sw[i1] * u1;
        }
        __syncthreads();
        // f = K a and the terms of the log marginal likelihood
        if (tid < N) {
            float acc = 0.f;
            for (int j = 0; j < N; ++j) acc += sK[tid * NP + j] * sb[j];
            sf[tid] = acc;
            st[tid] = lml_term(sy[tid], sb[tid], acc, sd[tid]);
        }
        __syncthreads();
        float lml = sum_le128(st, N, lane);          // every wave gets the same bits
        ++iters;
        if (lml - lml_prev < 1e-10f) break;
        lml_prev = lml;
    }

    const long po = prob * N;
    if (tid < N) {
        Fo[po + tid] = sf[tid];
        Go[po + tid] = sg[tid];
        Wo[po + tid] = sw[tid];
    }
    float* Lp = Lo + prob * (long)N * N;
    for (int idx = tid; idx < N * N; idx += T) {
        int i = idx / N, j = idx - i * N;
        Lp[idx] = j < i ? sA[i * NP + j] : (j == i ? sd[i] : 0.f);
    }
    if (tid == 0) {
        lml_o[prob] = lml_prev;
        it_o[prob] = iters;
    }
}

// Williams & Barber's approximation of the logistic sigmoid by five error functions, the constants of scikit-learn's _gpc.py
__device__ inline double probit_mixture(float mu_f, float var_f) {
    const double lambdas[5] = {0.41, 0.4, 0.37, 0.44, 0.39};
    const double coefs[5] = {-1854.8214151, 3516.89893646, 221.29346712, 128.12323805, -2010.49422654};
    const double kPi = 3.141592653589793;
    const double mu = (double)mu_f, var = (double)var_f;
    const double alpha = 1.0 / (2.0 * var);
    const double front = sqrt(kPi / alpha), back = 2.0 * sqrt(var * 2.0 * kPi);
    double sum = 0.0, csum = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        double integral = front * erf(lambdas[i] * mu * sqrt(alpha / (alpha + lambdas[i] * lambdas[i]))) / back;
        sum += coefs[i] * integral;
        csum += coefs[i];
    }
    return sum + 0.5 * csum;
}

__global__ __launch_bounds__(kQT) void gpc_predict_kernel(const float* __restrict__ Ks, long ksbs, long kscs, const float* __restrict__ kss,
                                                          long kssbs, long ksscs, const float* __restrict__ G, const float* __restrict__ W,
                                                          const float* __restrict__ Lc, float* __restrict__ mu_o, float* __restrict__ var_o,
                                                          float* __restrict__ prob_o, int* __restrict__ labels, int C, int M, int N,
                                                          int tiles) {
    extern __shared__ float lds[];
    const int NP = padded(N);
    float* sL = lds;
    float* sv = sL + N * NP;             // [N][kQS]: column `lane` is that lane's right-hand side, then its solution
    float* sg = sv + N * kQS;
    float* sw = sg + kVec;
    const int lane = threadIdx.x, b = blockIdx.x / tiles;
    const long q0 = (long)(blockIdx.x - b * tiles) * kQT;
    const int nq = (int)(M - q0 < kQT ? M - q0 : kQT);
    const long q = q0 + lane;
    double best = -INFINITY;
    int label = 0;
    float mu1 = 0.f;
    for (int c = 0; c < C; ++c) {
        const long pc = (long)b * C + c;
        const float* Lp = Lc + pc * (long)N * N;
        const float* Kp = Ks + (long)b * ksbs + (long)c * kscs + q0 * N;
        __syncthreads();
        stage_matrix<kQT>(sL, Lp, N, NP, lane);
        for (int idx = lane; idx < kQT * N; idx += kQT) {          // rows q0 .. q0 + nq - 1 of Ks, read along the rows; zeros for the lanes past M
            int qq = idx / N, n = idx - qq * N;
            sv[n * kQS + qq] = qq < nq ? Kp[idx] : 0.f;
        }
        for (int i = lane; i < N; i += kQT) {
            sg[i] = G[pc * N + i];
            sw[i] = W[pc * N + i];
        }
        __syncthreads();
        float mu = 0.f, acc = 0.f;
        for (int i = 0; i < N; ++i) {
            float ks = sv[i * kQS + lane];
            mu += ks * sg[i];
            float s = sw[i] * ks;
            for (int k = 0; k < i; ++k) s -= sL[i * NP + k] * sv[k * kQS + lane];
            float v = s / sL[i * NP + i];
            sv[i * kQS + lane] = v;
            acc += v * v;
        }
        if (lane < nq) {
            float var = kss[(long)b * kssbs + (long)c * ksscs + q] - acc;
            double p = probit_mixture(mu, var);
            const long o = pc * M + q;
            mu_o[o] = mu;
            var_o[o] = var;
            prob_o[o] = (float)p;
            if (p >= best) {             // the last of several equal maxima wins
                best = p;
                label = c;
            }
            mu1 = mu;
        }
    }
    if (labels && lane < nq) labels[(long)b * M + q] = C == 1 ? (mu1 > 0.f ? 1 : 0) : label;
}

}  // namespace

extern "C" int dkt_gpc_abi_version(void) { return DKT_GPC_ABI_VERSION; }

extern "C" int dkt_gpc_mode_f32(const float* K, long k_batch_stride, long k_class_stride, const float* Y, long y_batch_stride, float* f_hat,
                                float* g, float* w_sr, float* chol, float* lml, int* iters, int B, int C, int N, int max_iter, void* stream) {
    if (!K || !Y || !f_hat || !g || !w_sr || !chol || !lml || !iters || B <= 0 || C <= 0 || N <= 0 || max_iter <= 0) return DKT_ERR_BAD_ARG;
    if (k_batch_stride < 0 || k_class_stride < 0 || y_batch_stride < 0) return DKT_ERR_BAD_ARG;
    if (N > DKT_GPC_MAX_N || C > DKT_GPC_MAX_C) return DKT_ERR_SHAPE;
    if ((long long)B * C > 0x7fffffffLL) return DKT_ERR_TOO_LARGE;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = mode_lds_bytes(N);
    const dim3 grid((unsigned)(B * C));
    // a wave serves the small supports (5-way 1-shot and 5-shot: one barrier domain, more problems per CU), four waves the large ones
    if (N <= 32) {
        if (set_lds((const void*)gpc_mode_kernel<64>, lds) != DKT_OK) return DKT_ERR_LAUNCH;
        hipLaunchKernelGGL(gpc_mode_kernel<64>, grid, dim3(64), lds, st, K, k_batch_stride, k_class_stride, Y, y_batch_stride, f_hat, g, w_sr,
                           chol, lml, iters, C, N, max_iter);
    } else {
        if (set_lds((const void*)gpc_mode_kernel<256>, lds) != DKT_OK) return DKT_ERR_LAUNCH;
        hipLaunchKernelGGL(gpc_mode_kernel<256>, grid, dim3(256), lds, st, K, k_batch_stride, k_class_stride, Y, y_batch_stride, f_hat, g, w_sr,
                           chol, lml, iters, C, N, max_iter);
    }
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}

extern "C" int dkt_gpc_predict_f32(const float* Ks, long ks_batch_stride, long ks_class_stride, const float* kss, long kss_batch_stride,
                                   long kss_class_stride, const float* g, const float* w_sr, const float* chol, float* mu, float* var,
                                   float* prob, int* labels, int B, int C, int M, int N, void* stream) {
    if (!Ks || !kss || !g || !w_sr || !chol || !mu || !var || !prob || B <= 0 || C <= 0 || M <= 0 || N <= 0) return DKT_ERR_BAD_ARG;
    if (ks_batch_stride < 0 || ks_class_stride < 0 || kss_batch_stride < 0 || kss_class_stride < 0) return DKT_ERR_BAD_ARG;
    if (N > DKT_GPC_MAX_N || C > DKT_GPC_MAX_C) return DKT_ERR_SHAPE;
    const long long tiles = ((long long)M + kQT - 1) / kQT;
    if (tiles * B > 0x7fffffffLL) return DKT_ERR_TOO_LARGE;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = predict_lds_bytes(N);
    if (set_lds((const void*)gpc_predict_kernel, lds) != DKT_OK) return DKT_ERR_LAUNCH;
    hipLaunchKernelGGL(gpc_predict_kernel, dim3((unsigned)(tiles * B)), dim3(kQT), lds, st, Ks, ks_batch_stride, ks_class_stride, kss,
                       kss_batch_stride, kss_class_stride, g, w_sr, chol, mu, var, prob, labels, C, M, N, (int)tiles);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}
