/*
 * dkt_abi_x16.h -- C ABI of libdkt_x16.so (gfx950): the six front-end calls of dkt_abi.h for 16-bit trunk features, the output of a backbone
 * that runs in mixed precision (torch.autocast: bf16, or f16).
 *
 * Each entry point takes the arguments of its fp32 twin in dkt_abi.h, plus `xdtype` right after X:
 *   X  (and dX of the two backward calls) are `xdtype` elements (DKT_X_BF16 / DKT_X_F16), row-major [B,N,D], 8-byte aligned, D % 4 == 0;
 *   everything else -- gamma, beta, a, s, mean, rstd, var_unbiased, E, rnorm, Zn, W, dZn, the dgamma / dbeta parts -- is fp32 exactly as in dkt_abi.h.
 * X is widened to fp32 as it is loaded (exact); statistics, normalisation, the split Gram and the epilogues are the fp32 kernels' own arithmetic
 * (one template: csrc/dkt_frontend_kernels.h, csrc/dkt_frontend_big_kernels.h), so E, rnorm and the statistics are those of the fp32 call on the widened X.
 * dX is rounded to nearest-even into `xdtype` (overflow to +-inf), as Tensor.to(dtype).
 * Return values and the rest of the conventions: dkt_abi.h.  An unknown `xdtype`, a misaligned X / dX or D % 4 != 0 is DKT_ERR_BAD_ARG, checked on the
 * host before any launch.
 */
#ifndef DKT_ABI_X16_H
#define DKT_ABI_X16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKT_X16_ABI_VERSION 2 /* 2: + dkt_x16_env_value */

/* element type of X / dX */
#define DKT_X_BF16 1
#define DKT_X_F16 2

int dkt_x16_abi_version(void);
/* the library reads the environment switches of dkt_abi.h once; dkt_x16_reload_env() makes it read them again (as dkt_reload_env()) */
void dkt_x16_reload_env(void);
/* as dkt_env_value(): what this library's snapshot holds for DKT_<name> (ABI 2) */
const char* dkt_x16_env_value(const char* name);

/* twin: dkt_bn_stats_f32 */
int dkt_bn_stats_x16(const void* X, int xdtype, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                     float* a, float* s, float* var_unbiased, int B, int N, int D, void* stream);
/* twin: dkt_gram_bn_f32 (N <= 128) */
int dkt_gram_bn_x16(const void* X, int xdtype, const float* a, const float* s, long ab_bstride, float* E, float* rnorm,
                    int B, int N, int D, void* stream);
/* twin: dkt_gram_bn_train_f32 (N <= 128; the f16-split kernel and its fix-up pass) */
int dkt_gram_bn_train_x16(const void* X, int xdtype, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                          float* a, float* s, float* var_unbiased, float* E, float* rnorm, int B, int N, int D, void* stream);
/* twin: dkt_gram_bn_bwd_f32 (N <= 128); dX in xdtype */
int dkt_gram_bn_bwd_x16(const float* W, const float* E, const void* X, int xdtype, const float* a, const float* s, long ab_bstride,
                        const float* mean, const float* rstd, const float* rnorm, const float* ep_scale, void* dX,
                        float* dgamma_part, float* dbeta_part, int B, int N, int D, void* stream);
/* twin: dkt_affine_normalize_f32; Zn fp32 */
int dkt_affine_normalize_x16(const void* X, int xdtype, const float* a, const float* s, long ab_bstride, float* Zn, float* rnorm,
                             int B, int N, int D, void* stream);
/* twin: dkt_normalize_bn_bwd_f32; dX in xdtype */
int dkt_normalize_bn_bwd_x16(const float* dZn, const float* Zn, const void* X, int xdtype, const float* a, long a_bstride, const float* mean,
                             const float* rstd, const float* rnorm, void* dX, float* dgamma_part, float* dbeta_part, float* rowdot_ws,
                             int B, int N, int D, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DKT_ABI_X16_H */
