/*
 * dkt_abi_smk.h -- C ABI of libdkt_smk.so (gfx950): task-resident spectral-mixture kernels for many small regression tasks (the sine-wave
 * experiment: 10 or 5 support points of 40 features per task, a few hundred query points).
 *
 * The kernel is the one of dkt_smk_f32 (include/dkt_abi.h, csrc/dkt_spectral.hip):
 *
 *     E[i,j] = sum_q w_q  prod_d exp(-2 pi^2 (sigma_qd tau_d)^2) cos(2 pi mu_qd tau_d),     tau = a_i - b_j
 *
 * with weights [Q], means [Q,D], scales [Q,D] (constrained values), the product over d carried as (sign, log magnitude).  Here a workgroup holds
 * whole tasks (their rows and the Q x D hyper-parameters in LDS) and a lane computes whole entries, looping over d in order: no cross-lane
 * reduction, the results are bitwise reproducible.
 *
 * Limits (DKT_ERR_SHAPE outside them, before any launch): symmetric forward and backward N <= DKT_SMK_TASK_MAX_N; cross forward
 * M <= DKT_SMK_TASK_MAX_M and N <= DKT_SMK_TASK_MAX_N; D <= DKT_SMK_TASK_MAX_D; 1 <= Q <= DKT_SMK_TASK_MAX_Q.
 * Conventions, return values and streams: include/dkt_abi.h (device pointers, fp32 row-major, asynchronous on `stream`).
 */
#ifndef DKT_ABI_SMK_H
#define DKT_ABI_SMK_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKT_SMK_ABI_VERSION 1

/* a shape outside the limits of this library (the caller takes dkt_smk_f32 / dkt_smk_bwd_f32 of the product library instead) */
#ifndef DKT_ERR_SHAPE
#define DKT_ERR_SHAPE (-5)
#endif

#define DKT_SMK_TASK_MAX_N 32
#define DKT_SMK_TASK_MAX_M 256
#define DKT_SMK_TASK_MAX_D 64
#define DKT_SMK_TASK_MAX_Q 8

int dkt_smk_abi_version(void);

/* E[b] = k(x1[b], x2[b]): x1 [B,M,D], x2 [B,N,D] or NULL (symmetric, M == N: E[b] comes out exactly symmetric), E [B,M,N].  Only E is written. */
int dkt_smk_task_f32(const float* x1, const float* x2, const float* weights, const float* means, const float* scales, float* E, int B, int M,
                     int N, int D, int Q, void* stream);

/* bytes of the workspace dkt_smk_task_bwd_f32 needs (per-task partials of the hyper-parameter gradients) */
size_t dkt_smk_task_workspace_bytes(int B, int N, int D, int Q);

/* Chain rule of the symmetric matrix E[b] = k(x[b], x[b]) given gE [B,N,N] (any matrix, not necessarily symmetric): dx [B,N,D] per task;
 * dweights [Q], dmeans [Q,D], dscales [Q,D] summed over the B tasks in a fixed order (bitwise reproducible).  The mixture terms are recomputed.
 * ws: device workspace of dkt_smk_task_workspace_bytes(B, N, D, Q) bytes, 4-byte aligned.  Two launches. */
int dkt_smk_task_bwd_f32(const float* gE, const float* x, const float* weights, const float* means, const float* scales, float* dx,
                         float* dweights, float* dmeans, float* dscales, void* ws, int B, int N, int D, int Q, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DKT_ABI_SMK_H */
