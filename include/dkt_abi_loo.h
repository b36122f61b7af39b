/*
 * dkt_abi_loo.h -- C ABI of libdkt_loo.so (gfx950): the leave-one-out predictive log likelihood of exact GP regression (Rasmussen & Williams,
 * GPML, section 5.4.2) and its gradients, for the one-vs-rest class models of B episodes.  docs/LOO.md has the formulas and the conventions.
 *
 * One call, one launch: factorisation (with the jitter ladder of dkt_mll_f32), inverse, the N leave-one-out predictions and the gradients run
 * inside the kernel, nothing is read back.  All arithmetic is plain fp32 (no 16-bit splits), no atomics: the call is bitwise reproducible.
 *
 * Limits (DKT_ERR_SHAPE outside them, before any launch): 1 <= N <= DKT_LOO_MAX_N, 1 <= C <= DKT_LOO_MAX_C.
 * Conventions, return values and streams: include/dkt_abi.h (device pointers, fp32 row-major, asynchronous on `stream`).  Strides count elements.
 */
#ifndef DKT_ABI_LOO_H
#define DKT_ABI_LOO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKT_LOO_ABI_VERSION 1

#ifndef DKT_ERR_SHAPE
#define DKT_ERR_SHAPE (-5)
#endif

#define DKT_LOO_MAX_N 127
#define DKT_LOO_MAX_C 32

#define DKT_LOO_WANT_GRAD 1u /* flags: write W, dsv, dmean, dnoise */

int dkt_loo_abi_version(void);

/* Problem (b, c): base matrix E + b e_bstride + c e_cstride ([N,N], symmetric: the lower triangle is read; e_cstride 0: the C class models of an
 * episode share one E, e_cstride N*N: one per class; anything else is DKT_ERR_BAD_ARG), targets Y + b y_bstride + c N (y_bstride 0: every
 * episode has the same targets [C,N]); sv, mean, noise [C]; cls_weight [C] or NULL (= 1).
 *     K = sv_c E + (noise_c + jitter) I,  A = K^-1,  alpha = A (y - mean_c),  d = diag A,
 *     mu_loo_i = y_i - alpha_i / d_i,  var_loo_i = 1 / d_i,  loo = sum_i [ 1/2 log d_i - alpha_i^2 / (2 d_i) - 1/2 log 2 pi ].
 * jitter: 0 first, then the total diagonal jitter jitter0 * 10^i, i < max_tries, until the fp32 Cholesky factorisation meets no pivot that is
 * not finite and positive; decided per matrix inside the kernel.  jitter_used [B,C] is the rung taken, info [B,C] 0 -- or, when every rung
 * failed, 1 + the index of the last attempt's failing pivot: every output of that problem is NaN then (a shared W[b] too), the other problems
 * are as they would be without it.
 * Written: loo [B,C] (unweighted), alpha, mu_loo, var_loo [B,C,N], jitter_used, info.
 * flags & DKT_LOO_WANT_GRAD (the four pointers may be NULL without it), with p_i = 1/(2 d_i) + alpha_i^2 / (2 d_i^2), q_i = alpha_i / d_i, r = A q
 * and G = -A diag(p) A + 1/2 (alpha r^T + r alpha^T) = d loo / d K (symmetric):
 *     dsv = sum_ij G_ij E_ij,  dnoise = tr G,  dmean = sum_i r_i      [B,C], raw (no cls_weight), as dkt_mll_f32 reports its own;
 *     W = cls_weight_c sv_c G_c: [B,C,N,N] for a per-class E, [B,N,N] = the sum over the classes in index order for a shared E.  Bitwise symmetric.
 * No workspace. */
int dkt_loo_f32(const float* E, long e_bstride, long e_cstride, const float* Y, long y_bstride, const float* sv, const float* mean,
                const float* noise, const float* cls_weight, int B, int C, int N, float jitter0, int max_tries, unsigned flags, float* loo,
                float* alpha, float* mu_loo, float* var_loo, float* W, float* dsv, float* dmean, float* dnoise, float* jitter_used,
                int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DKT_ABI_LOO_H */
