// dkt_frontend.hip -- the BNCosSim front half of the deep kernel fused into the Gram build:
//   reference  z = trunk(x) ending in bn_out = BatchNorm1d(D)   (methods/DKT.py:48)
//              z = F.normalize(z, p=2, dim=1)                   (methods/DKT.py:141-142, 174-175, 236-237)
//              K = LinearKernel(z, z)                           (methods/DKT.py:375-378)
// here       dkt_bn_stats_f32   : per-episode batch statistics of the raw trunk output X[b] (train mode), folded into
//                                 an affine map  y = a x + s   (a = gamma rstd, s = beta - mean a)
//            dkt_gram_bn_f32    : E = Zn Zn^T with Zn_i = y_i / max(||y_i||, 1e-12) -- the affine map is applied while the
//                                 slice is staged, the row norms come out of the diagonal of G' = Y Y^T, Zn is never written
// (dkt_gram_bn_bwd_f32 is the matching backward.)  The kernels live in dkt_frontend_kernels.h, templated on the element type of X / dX: this file
// instantiates fp32 (the product), dkt_frontend_x16.hip bf16 / f16 (libdkt_x16.so).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "dkt_common.h"
#include "dkt_tiles.h"
#include "dkt_split.h"
#include "dkt_frontend_kernels.h"
#include "../../include/dkt_abi.h"

// Episode-resident squared-distance / RBF build of dkt_gram_f32 (symmetric, 32 < N <= 128, D % 4 == 0, 16-byte aligned Z, a batch that
// fills the GPU); returns false when it does not apply (the generic 64 x 64-tile kernel then runs).
bool dkt_gram_dist_ep_launch(const float* Z, float* E, int B, int N, int D, int kind, const float* lengthscale, hipStream_t st) {
    const int minb = dkt_env_int(DKT_SW_GRAM_EP_MINB, 64);          // (64 here, 32 for the linear kernels of dkt_gram_ep.hip)
    const bool on = dkt_env_on(DKT_SW_GRAM_DIST_EP);
    if (!on || N <= 32 || N > 128 || (D & 3) || ((uintptr_t)Z & 15) || B < minb || !lengthscale) return false;
    if (kind != DKT_KERNEL_RBF && kind != DKT_KERNEL_SQDIST) return false;
    BnTrainOut bo{};
    bo.lengthscale = lengthscale;
    bo.epi = (kind == DKT_KERNEL_RBF) ? 2 : 1;
    gram_bn_dispatch<float>(Z, Z, Z, 0, E, nullptr, B, N, D, st, &bo);
    return true;
}

extern "C" int dkt_bn_stats_f32(const float* X, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                                float* a, float* s, float* var_unbiased, int B, int N, int D, void* stream) {
    if (!X || !mean || !rstd || !a || !s || B <= 0 || N <= 0 || D <= 0) return DKT_ERR_BAD_ARG;
    if ((D & 3) || ((uintptr_t)X & 15)) return DKT_ERR_BAD_ARG;
    if (B > 65535) return DKT_ERR_TOO_LARGE;
    dim3 grid((D + 255) / 256, B);
    hipLaunchKernelGGL(bn_stats_kernel<float>, grid, dim3(1024), 0, (hipStream_t)stream, X, gamma, beta, eps, mean, rstd, a, s, var_unbiased, N, D);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}

extern "C" int dkt_gram_bn_f32(const float* X, const float* a, const float* s, long ab_bstride, float* E, float* rnorm,
                               int B, int N, int D, void* stream) {
    if (!X || !a || !s || !E || !rnorm || B <= 0 || N <= 0 || D <= 0) return DKT_ERR_BAD_ARG;
    if ((D & 3) || ((uintptr_t)X & 15) || ((uintptr_t)a & 15) || ((uintptr_t)s & 15) || (ab_bstride & 3)) return DKT_ERR_BAD_ARG;
    if (N > 128) return DKT_ERR_TOO_LARGE;
    return gram_bn_dispatch<float>(X, a, s, ab_bstride, E, rnorm, B, N, D, (hipStream_t)stream, nullptr);
}

extern "C" int dkt_gram_bn_train_f32(const float* X, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                                     float* a, float* s, float* var_unbiased, float* E, float* rnorm, int B, int N, int D, void* stream) {
    if (!X || !mean || !rstd || !a || !s || !E || !rnorm || B <= 0 || N <= 0 || D <= 0) return DKT_ERR_BAD_ARG;
    if ((D & 3) || ((uintptr_t)X & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15)) return DKT_ERR_BAD_ARG;
    if (((uintptr_t)mean & 15) || ((uintptr_t)rstd & 15) || ((uintptr_t)a & 15) || ((uintptr_t)s & 15) || ((uintptr_t)var_unbiased & 15)) return DKT_ERR_BAD_ARG;
    if (N > 128) return DKT_ERR_TOO_LARGE;
    BnTrainOut bo{};
    bo.mean = mean; bo.rstd = rstd; bo.a = a; bo.s = s; bo.var_unbiased = var_unbiased;
    bo.eps = eps; bo.has_gamma = gamma != nullptr; bo.has_beta = beta != nullptr;
    // absent gamma / beta: any valid pointer keeps the descriptor legal, the values are ignored (has_* = 0)
    return gram_bn_dispatch<float>(X, gamma ? gamma : X, beta ? beta : X, 0, E, rnorm, B, N, D, (hipStream_t)stream, &bo);
}

extern "C" int dkt_gram_bn_bwd_f32(const float* W, const float* E, const float* X, const float* a, const float* s, long ab_bstride,
                                   const float* mean, const float* rstd, const float* rnorm, const float* ep_scale, float* dX,
                                   float* dgamma_part, float* dbeta_part, int B, int N, int D, void* stream) {
    if (!W || !E || !X || !a || !s || !rnorm || !dX || B <= 0 || N <= 0 || D <= 0) return DKT_ERR_BAD_ARG;
    const bool train_bn = mean != nullptr;
    if (train_bn && (!rstd || !dgamma_part || !dbeta_part)) return DKT_ERR_BAD_ARG;
    if ((D & 3) || ((uintptr_t)X & 15) || ((uintptr_t)dX & 15) || ((uintptr_t)a & 15) || ((uintptr_t)s & 15) || (ab_bstride & 3)) return DKT_ERR_BAD_ARG;
    if (N > 128) return DKT_ERR_TOO_LARGE;
    return gram_bn_bwd_dispatch<float>(W, E, X, a, s, ab_bstride, mean, rstd, rnorm, ep_scale, dX, dgamma_part, dbeta_part, B, N, D, train_bn, (hipStream_t)stream);
}
