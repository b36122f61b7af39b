/*
 * dkt_abi_gpc.h -- C ABI of libdkt_gpc.so (gfx950): binary Gaussian-process classification with the Laplace approximation (Rasmussen & Williams,
 * GPML, algorithms 3.1 and 3.2), for the one-vs-rest class models of a test episode.  docs/LAPLACE.md has the algorithm and the conventions.
 *
 * Two calls.  dkt_gpc_mode_f32 finds the posterior mode of B x C independent binary problems in one launch: the Newton loop and its stopping
 * test run inside the kernel (a workgroup per problem, K resident in LDS), nothing is read back between iterations.  dkt_gpc_predict_f32 turns
 * the mode into latent mean, latent variance, the class probability (the five-term probit mixture of Williams & Barber, summed in double) and
 * the one-vs-rest label, in one launch.  All other arithmetic is plain fp32 (no 16-bit splits).  Both calls are bitwise reproducible.
 *
 * Limits (DKT_ERR_SHAPE outside them, before any launch): 1 <= N <= DKT_GPC_MAX_N, 1 <= C <= DKT_GPC_MAX_C.  M is not limited.
 * Conventions, return values and streams: include/dkt_abi.h (device pointers, fp32 row-major, asynchronous on `stream`).  Strides count elements.
 */
#ifndef DKT_ABI_GPC_H
#define DKT_ABI_GPC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKT_GPC_ABI_VERSION 1

#ifndef DKT_ERR_SHAPE
#define DKT_ERR_SHAPE (-5)
#endif

#define DKT_GPC_MAX_N 127
#define DKT_GPC_MAX_C 32

int dkt_gpc_abi_version(void);

/* Posterior mode of problem (b, c): prior covariance K + b k_batch_stride + c k_class_stride ([N,N]; k_class_stride 0: the C problems of an
 * episode share one K), targets in {0,1} at Y + b y_batch_stride + c N (y_batch_stride 0: every episode has the same targets [C,N]).
 * From f = 0, at most max_iter (>= 1) times:
 *     pi = sigmoid(f), W = pi (1 - pi), L = chol(I + W^1/2 K W^1/2), b = W f + (y - pi), a = b - W^1/2 L^-T L^-1 W^1/2 K b, f <- K a,
 *     lml = -1/2 a.f - sum log(1 + exp(-(2y - 1) f)) - sum log L_ii;         stop when lml - lml_prev < 1e-10.
 * Written per problem: f_hat [B,C,N] the last f; g [B,C,N] = y - pi, w_sr [B,C,N] = W^1/2 and chol [B,C,N,N] = L (lower triangle, zeros above)
 * with pi taken at the START of the last executed iteration; lml [B,C] the value of the iteration before the last one (the last one's when
 * max_iter ran out); iters [B,C] the number of executed iterations. */
int dkt_gpc_mode_f32(const float* K, long k_batch_stride, long k_class_stride, const float* Y, long y_batch_stride, float* f_hat, float* g,
                     float* w_sr, float* chol, float* lml, int* iters, int B, int C, int N, int max_iter, void* stream);

/* Prediction at M query points from g, w_sr, chol of dkt_gpc_mode_f32: cross kernel Ks + b ks_batch_stride + c ks_class_stride ([M,N]) and prior
 * variance kss + b kss_batch_stride + c kss_class_stride ([M]); a class stride of 0 shares them between the classes.
 *     mu = Ks g,   var = kss - |L^-1 (w_sr * Ks^T)|^2                                                          (fp32; mu, var [B,C,M])
 *     prob = sum_i COEFS_i sqrt(pi / alpha) erf(LAMBDAS_i mu sqrt(alpha / (alpha + LAMBDAS_i^2))) / (2 sqrt(2 pi var)) + 1/2 sum COEFS,
 *            alpha = 1 / (2 var)                                                    (evaluated in double from the fp32 mu, var; prob [B,C,M])
 *     labels [B,M] (int32, may be NULL): C >= 2: the class of the largest prob, the LAST of several equal maxima; C == 1: mu > 0. */
int dkt_gpc_predict_f32(const float* Ks, long ks_batch_stride, long ks_class_stride, const float* kss, long kss_batch_stride,
                        long kss_class_stride, const float* g, const float* w_sr, const float* chol, float* mu, float* var, float* prob,
                        int* labels, int B, int C, int M, int N, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DKT_ABI_GPC_H */
