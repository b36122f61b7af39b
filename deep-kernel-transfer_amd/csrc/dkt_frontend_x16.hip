// dkt_frontend_x16.hip -- libdkt_x16.so: the front-end kernels of dkt_frontend.hip / dkt_frontend_big.hip instantiated for 16-bit trunk features
// (XT = __bf16 / _Float16: a backbone under torch.autocast), behind the six entry points of include/dkt_abi_x16.h.  Same templates as the product's
// fp32 kernels; only the loads of X (8 bytes per 4 elements, widened exactly) and the stores of dX (rounded to nearest-even) differ.  A separate shared
// object: the product library's kernel list and ABI stay as they are.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "dkt_common.h"
#include "dkt_frontend_kernels.h"
#include "dkt_frontend_big_kernels.h"
#include "../../include/dkt_abi.h"
#include "../../include/dkt_abi_x16.h"

namespace {

bool xdtype_ok(int xdtype) { return xdtype == DKT_X_BF16 || xdtype == DKT_X_F16; }
bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int dkt_x16_abi_version(void) { return DKT_X16_ABI_VERSION; }

extern "C" void dkt_x16_reload_env(void) { dkt_env_reload(); }
extern "C" const char* dkt_x16_env_value(const char* name) { return dkt_env_by_name(name); }

extern "C" int dkt_bn_stats_x16(const void* X, int xdtype, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                                float* a, float* s, float* var_unbiased, int B, int N, int D, void* stream) {
    if (!X || !mean || !rstd || !a || !s || B <= 0 || N <= 0 || D <= 0 || !xdtype_ok(xdtype)) return DKT_ERR_BAD_ARG;
    if ((D & 3) || !al8(X)) return DKT_ERR_BAD_ARG;
    if (B > 65535) return DKT_ERR_TOO_LARGE;
    dim3 grid((D + 255) / 256, B);
    hipStream_t st = (hipStream_t)stream;
    if (xdtype == DKT_X_BF16)
        hipLaunchKernelGGL(bn_stats_kernel<__bf16>, grid, dim3(1024), 0, st, (const __bf16*)X, gamma, beta, eps, mean, rstd, a, s, var_unbiased, N, D);
    else
        hipLaunchKernelGGL(bn_stats_kernel<_Float16>, grid, dim3(1024), 0, st, (const _Float16*)X, gamma, beta, eps, mean, rstd, a, s, var_unbiased, N, D);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}

extern "C" int dkt_gram_bn_x16(const void* X, int xdtype, const float* a, const float* s, long ab_bstride, float* E, float* rnorm,
                               int B, int N, int D, void* stream) {
    if (!X || !a || !s || !E || !rnorm || B <= 0 || N <= 0 || D <= 0 || !xdtype_ok(xdtype)) return DKT_ERR_BAD_ARG;
    if ((D & 3) || !al8(X) || !al16(a) || !al16(s) || (ab_bstride & 3)) return DKT_ERR_BAD_ARG;
    if (N > 128) return DKT_ERR_TOO_LARGE;
    hipStream_t st = (hipStream_t)stream;
    if (xdtype == DKT_X_BF16) return gram_bn_dispatch<__bf16>((const __bf16*)X, a, s, ab_bstride, E, rnorm, B, N, D, st, nullptr);
    return gram_bn_dispatch<_Float16>((const _Float16*)X, a, s, ab_bstride, E, rnorm, B, N, D, st, nullptr);
}

extern "C" int dkt_gram_bn_train_x16(const void* X, int xdtype, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                                     float* a, float* s, float* var_unbiased, float* E, float* rnorm, int B, int N, int D, void* stream) {
    if (!X || !mean || !rstd || !a || !s || !E || !rnorm || B <= 0 || N <= 0 || D <= 0 || !xdtype_ok(xdtype)) return DKT_ERR_BAD_ARG;
    if ((D & 3) || !al8(X) || !al16(gamma) || !al16(beta)) return DKT_ERR_BAD_ARG;
    if (!al16(mean) || !al16(rstd) || !al16(a) || !al16(s) || !al16(var_unbiased)) return DKT_ERR_BAD_ARG;
    if (N > 128) return DKT_ERR_TOO_LARGE;
    BnTrainOut bo{};
    bo.mean = mean; bo.rstd = rstd; bo.a = a; bo.s = s; bo.var_unbiased = var_unbiased;
    bo.eps = eps; bo.has_gamma = gamma != nullptr; bo.has_beta = beta != nullptr;
    // absent gamma / beta: any valid pointer keeps the descriptor legal, the values are ignored (has_* = 0)
    const float* g = gamma ? gamma : mean;
    const float* bt = beta ? beta : mean;
    hipStream_t st = (hipStream_t)stream;
    if (xdtype == DKT_X_BF16) return gram_bn_dispatch<__bf16>((const __bf16*)X, g, bt, 0, E, rnorm, B, N, D, st, &bo);
    return gram_bn_dispatch<_Float16>((const _Float16*)X, g, bt, 0, E, rnorm, B, N, D, st, &bo);
}

extern "C" int dkt_gram_bn_bwd_x16(const float* W, const float* E, const void* X, int xdtype, const float* a, const float* s, long ab_bstride,
                                   const float* mean, const float* rstd, const float* rnorm, const float* ep_scale, void* dX,
                                   float* dgamma_part, float* dbeta_part, int B, int N, int D, void* stream) {
    if (!W || !E || !X || !a || !s || !rnorm || !dX || B <= 0 || N <= 0 || D <= 0 || !xdtype_ok(xdtype)) return DKT_ERR_BAD_ARG;
    const bool train_bn = mean != nullptr;
    if (train_bn && (!rstd || !dgamma_part || !dbeta_part)) return DKT_ERR_BAD_ARG;
    if ((D & 3) || !al8(X) || !al8(dX) || !al16(a) || !al16(s) || (ab_bstride & 3)) return DKT_ERR_BAD_ARG;
    if (N > 128) return DKT_ERR_TOO_LARGE;
    hipStream_t st = (hipStream_t)stream;
    if (xdtype == DKT_X_BF16)
        return gram_bn_bwd_dispatch<__bf16>(W, E, (const __bf16*)X, a, s, ab_bstride, mean, rstd, rnorm, ep_scale, (__bf16*)dX, dgamma_part, dbeta_part,
                                            B, N, D, train_bn, st);
    return gram_bn_bwd_dispatch<_Float16>(W, E, (const _Float16*)X, a, s, ab_bstride, mean, rstd, rnorm, ep_scale, (_Float16*)dX, dgamma_part, dbeta_part,
                                          B, N, D, train_bn, st);
}

extern "C" int dkt_affine_normalize_x16(const void* X, int xdtype, const float* a, const float* s, long ab_bstride, float* Zn, float* rnorm,
                                        int B, int N, int D, void* stream) {
    if (!X || !a || !s || !Zn || !rnorm || B <= 0 || N <= 0 || D <= 0 || !xdtype_ok(xdtype)) return DKT_ERR_BAD_ARG;
    if ((D & 3) || !al8(X) || !al16(Zn) || !al16(a) || !al16(s) || (ab_bstride & 3) || ab_bstride < 0) return DKT_ERR_BAD_ARG;
    const long rows = (long)B * N;
    if ((rows + 3) / 4 > 0x7fffffffL) return DKT_ERR_TOO_LARGE;
    hipStream_t st = (hipStream_t)stream;
    if (xdtype == DKT_X_BF16) return affine_normalize_launch<__bf16>((const __bf16*)X, a, s, ab_bstride, Zn, rnorm, rows, N, D, st);
    return affine_normalize_launch<_Float16>((const _Float16*)X, a, s, ab_bstride, Zn, rnorm, rows, N, D, st);
}

extern "C" int dkt_normalize_bn_bwd_x16(const float* dZn, const float* Zn, const void* X, int xdtype, const float* a, long a_bstride, const float* mean,
                                        const float* rstd, const float* rnorm, void* dX, float* dgamma_part, float* dbeta_part, float* rowdot_ws,
                                        int B, int N, int D, void* stream) {
    if (!dZn || !Zn || !a || !rnorm || !dX || !rowdot_ws || B <= 0 || N <= 0 || D <= 0 || !xdtype_ok(xdtype)) return DKT_ERR_BAD_ARG;
    const bool train = mean != nullptr;
    if (train && (!X || !rstd || !dgamma_part || !dbeta_part)) return DKT_ERR_BAD_ARG;
    if ((D & 3) || !al16(dZn) || !al16(Zn) || !al8(X) || !al8(dX) || !al16(a) || (a_bstride & 3) || a_bstride < 0) return DKT_ERR_BAD_ARG;
    if (train && (!al16(mean) || !al16(rstd) || !al16(dgamma_part) || !al16(dbeta_part))) return DKT_ERR_BAD_ARG;
    if (N > 1024) return DKT_ERR_TOO_LARGE;                                  // the slab's dY lives in LDS: 128 B per row
    const long rows = (long)B * N;
    const int nslab = (D + 31) / 32;
    if ((rows + 3) / 4 > 0x7fffffffL || (long)B * nslab > 0x7fffffffL) return DKT_ERR_TOO_LARGE;
    hipStream_t st = (hipStream_t)stream;
    if (xdtype == DKT_X_BF16)
        return normalize_bn_bwd_launch<__bf16>(dZn, Zn, (const __bf16*)X, a, a_bstride, mean, rstd, rnorm, (__bf16*)dX, dgamma_part, dbeta_part, rowdot_ws,
                                               B, N, D, train, st);
    return normalize_bn_bwd_launch<_Float16>(dZn, Zn, (const _Float16*)X, a, a_bstride, mean, rstd, rnorm, (_Float16*)dX, dgamma_part, dbeta_part, rowdot_ws,
                                             B, N, D, train, st);
}
