/*
 * dkt_abi_post.h -- C ABI of libdkt_post.so (gfx950): the JOINT posterior of exact GP regression at a set of query points (Rasmussen & Williams,
 * GPML, section 2.2, eq. 2.22-2.24): mean, full predictive covariance, its Cholesky factor, the joint and the marginal predictive log likelihood of
 * held-out targets, and function draws, for the C models of B episodes.  docs/POSTERIOR.md has the formulas and the conventions.
 *
 * One call, one launch: both factorisations (each with the jitter ladder of dkt_mll_f32), the triangular solves, the covariance and everything read
 * off its factor run inside the kernel, nothing is read back.  All arithmetic is plain fp32 (no 16-bit splits; the dot products of V^T V, which
 * cancel against sv E_qq, are summed in double and rounded once), no atomics, every sum in a fixed order: the call is bitwise reproducible.
 *
 * Limits (DKT_ERR_SHAPE outside them, before any launch): 1 <= N <= DKT_POST_MAX_N, 1 <= M <= DKT_POST_MAX_M, 1 <= C <= DKT_POST_MAX_C, 0 <= S.
 * Conventions, return values and streams: include/dkt_abi.h (device pointers, fp32 row-major, asynchronous on `stream`).  Strides count elements.
 */
#ifndef DKT_ABI_POST_H
#define DKT_ABI_POST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKT_POST_ABI_VERSION 1

#ifndef DKT_ERR_SHAPE
#define DKT_ERR_SHAPE (-5)
#endif

#define DKT_POST_MAX_N 127
#define DKT_POST_MAX_M 127
#define DKT_POST_MAX_C 32

int dkt_post_abi_version(void);

/* The scratch dkt_posterior_f32 needs: B C M M floats for Sigma when `cov` is not asked for (want_cov 0), nothing otherwise.  0 for shapes outside
 * the limits. */
size_t dkt_posterior_workspace_bytes(int B, int C, int M, int want_cov);

/* Problem (b, c), N support rows and M query rows: base matrices E_ss + b ss_bstride + c ss_cstride ([N,N], symmetric: the lower triangle is read),
 * E_qs + b qs_bstride + c qs_cstride ([M,N]: query rows against support rows) and E_qq + b qq_bstride + c qq_cstride ([M,M], symmetric: the lower
 * triangle is read); a class stride of 0: the C models of an episode share the matrix, of the matrix' own size (N N, M N, M M): one per class;
 * anything else is DKT_ERR_BAD_ARG.  Targets Y + b y_bstride + c N (y_bstride 0: every episode has the same targets [C,N]); sv, mean, noise [C].
 * Yq [B,C,M] or NULL: held-out targets of the query rows; eps [B,C,S,M] or NULL: standard-normal numbers, the caller's.  with_noise 0 | 1.
 *     K  = sv_c E_ss + (noise_c + jitter_s) I = L L^T,   t = L^-1 (y - mean_c),   V = L^-1 (sv_c E_qs^T)   [N x M]
 *     mu = mean_c + V^T t,   Sigma = sv_c E_qq - V^T V + (with_noise ? noise_c : 0) I,   Sigma + jitter_q I = R R^T
 *     logp = -1/2 |R^-1 (yq - mu)|^2 - sum_i log R_ii - M/2 log 2 pi        the joint predictive log likelihood of Yq
 *     lpd  = sum_i log N(yq_i | mu_i, Sigma_ii)                              its marginal counterpart (no jitter_q)
 *     samples[s] = mu + R eps[s]
 * jitter_s, jitter_q: 0 first, then the total diagonal jitter jitter0 * 10^i, i < max_tries, until the fp32 Cholesky factorisation meets no pivot
 * that is not finite and positive; decided per matrix inside the kernel, for K and for Sigma apart.
 * Written, each unless its pointer is NULL: mu [B,C,M]; cov [B,C,M,M] = Sigma (without jitter_q; bitwise symmetric); chol_q [B,C,M,M] = R (lower
 * triangle, zeros above); logp, lpd [B,C] (they need Yq: DKT_ERR_BAD_ARG without); samples [B,C,S,M] (S >= 1 needs eps and samples, S = 0 neither:
 * DKT_ERR_BAD_ARG otherwise).  Always written: jitter_s, jitter_q [B,C], the rungs taken, and info_s, info_q [B,C]: 0, or 1 + the failing pivot of
 * the last rung when every rung failed.
 *     info_s != 0: every output of the problem is NaN (info_q = 1, jitter_q = the last rung: the ladder over a NaN Sigma);
 *     info_q != 0: chol_q, logp and samples are NaN; mu, cov and lpd are valid.
 * The other problems of the call are as they would be without the failed one.
 * workspace: dkt_posterior_workspace_bytes(B, C, M, cov != NULL) bytes (DKT_ERR_WORKSPACE when smaller; may be NULL when that is 0). */
int dkt_posterior_f32(const float* E_ss, long ss_bstride, long ss_cstride, const float* E_qs, long qs_bstride, long qs_cstride, const float* E_qq,
                      long qq_bstride, long qq_cstride, const float* Y, long y_bstride, const float* sv, const float* mean, const float* noise,
                      const float* Yq, const float* eps, int B, int C, int N, int M, int S, int with_noise, float jitter0, int max_tries,
                      float* mu, float* cov, float* chol_q, float* logp, float* lpd, float* samples, float* jitter_s, float* jitter_q,
                      int32_t* info_s, int32_t* info_q, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DKT_ABI_POST_H */
