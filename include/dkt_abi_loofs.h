/*
 * dkt_abi_loofs.h -- C ABI of libdkt_loofs.so (gfx950): the leave-one-out predictive log likelihood of exact GP regression (include/dkt_abi_loo.h) for
 * the LINEAR kernels in FEATURE space, K = sv_c Z Z^T + (noise_c + jitter) I with Z [N,D], D <= 64 and any number of rows N: no N x N matrix is
 * formed, the episode's rows are streamed in blocks of DKT_LOOFS_ROWS.  docs/LOOFS.md has the formulas, the kernel and the measurements.
 *
 * One call, one launch, a workgroup per episode: S = Z^T Z once per episode, then its class models one after the other.  All arithmetic is plain
 * fp32 on the VALU (no 16-bit splits), no atomics: the call is bitwise reproducible, and a batch equals its episodes one by one.
 *
 * Limits (DKT_ERR_SHAPE outside them, before any launch): N >= 1, 1 <= D <= DKT_LOOFS_MAX_D, D % 4 == 0, 1 <= C <= DKT_LOOFS_MAX_C.
 * Conventions, return values and streams: include/dkt_abi.h (device pointers, fp32 row-major, asynchronous on `stream`).  Strides count elements.
 */
#ifndef DKT_ABI_LOOFS_H
#define DKT_ABI_LOOFS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKT_LOOFS_ABI_VERSION 1

#ifndef DKT_ERR_SHAPE
#define DKT_ERR_SHAPE (-5)
#endif

#define DKT_LOOFS_MAX_D 64
#define DKT_LOOFS_MAX_C 32
#define DKT_LOOFS_ROWS 64 /* R: rows of Z a workgroup holds at a time */

#define DKT_LOOFS_WANT_GRAD 1u /* flags: write dZ, dsv, dmean, dnoise */

int dkt_loofs_abi_version(void);

/* Bytes of workspace dkt_loofs_f32 needs for these sizes (S of every episode); 0 outside the limits. */
size_t dkt_loofs_workspace_bytes(int B, int C, int N, int D);

/* Problem (b, c): rows Z + b N D ([N,D], 16-byte aligned), targets Y + b y_bstride + c N (y_bstride 0: every episode has the same targets [C,N]);
 * sv, mean, noise [C]; cls_weight [C] or NULL (= 1).  With s = noise_c + jitter, v = sv_c, lam = s / v, r = y - mean_c:
 *     S = Z^T Z,  A = S + lam I,  G = A^-1,  p = Z^T r,  w = G p,
 *     alpha_i = (r_i - z_i.w) / s  (= (K^-1 r)_i),   h_i = z_i^T G z_i,   k_i = (1 - h_i) / s  (= (K^-1)_ii),
 *     mu_loo_i = y_i - alpha_i / k_i,  var_loo_i = 1 / k_i,  loo = sum_i [ 1/2 log k_i - alpha_i^2 / (2 k_i) - 1/2 log 2 pi ].
 * jitter: the ladder of dkt_loo_f32 -- 0 first, then the total diagonal jitter jitter0 * 10^i, i < max_tries -- per (episode, class), inside the
 * kernel, until the fp32 Cholesky factorisation of A [D,D] meets no pivot that is not finite and positive (and, for N > D, s > 0: K has the
 * eigenvalue s there).  jitter_used [B,C] is the rung taken, info [B,C] 0 -- or, when every rung failed, 1 + the index of the last attempt's
 * failing pivot (1 + D for s <= 0): every output of that problem is NaN then, and so is the dZ of its episode; the other episodes are as they
 * would be without it.
 * Written: loo [B,C] (unweighted), alpha, mu_loo, var_loo [B,C,N], jitter_used, info.
 * flags & DKT_LOOFS_WANT_GRAD (the four pointers may be NULL without it):
 *     dsv, dmean, dnoise [B,C]: d loo / d sv_c, d mean_c, d noise_c, raw (no cls_weight), as dkt_loo_f32 reports its own;
 *     dZ [B,N,D] (16-byte aligned) = sum_c cls_weight_c d loo_c / d Z, the classes in index order.
 * workspace: dkt_loofs_workspace_bytes(B, C, N, D) bytes, 16-byte aligned (DKT_ERR_WORKSPACE when NULL or short). */
int dkt_loofs_f32(const float* Z, const float* Y, long y_bstride, const float* sv, const float* mean, const float* noise,
                  const float* cls_weight, int B, int C, int N, int D, float jitter0, int max_tries, unsigned flags, float* loo, float* alpha,
                  float* mu_loo, float* var_loo, float* dZ, float* dsv, float* dmean, float* dnoise, float* jitter_used, int32_t* info,
                  void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DKT_ABI_LOOFS_H */
