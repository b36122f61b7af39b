// dkt_frontend_big.hip -- the front end of a training episode with MORE than 128 rows (the 20-way shapes of train.py:132-133: N = 420): train-mode
// BatchNorm1d + F.normalize in front of the large-N Gram kernels, and the way back, as three streaming kernels.
//
// Replaces bn_out in train mode + F.normalize (reference methods/DKT.py:48, 141-142) and autograd through both (loss.backward(), DKT.py:163) where the
// episode-resident fused kernels of dkt_frontend.hip (N <= 128: the normalised features never leave the chip) do not apply: the large-N Gram kernels need
// unit rows as their INPUT (they scale-split them to f16), so Zn is written once -- but by ONE kernel instead of the seven element-wise / reduction kernels
// torch runs for the same two modules (9.4 ms per 1024 episodes of 420 x 512 features, a third of the whole step: profiles/r04/v13_front_end_large_n.log).
//
//   forward : dkt_bn_stats_f32 (column statistics, folded into a / s)  ->  dkt_affine_normalize_f32:  y = a x + s,  rn = 1 / max(|y|, 1e-12),  Zn = y rn
//   backward: dkt_normalize_bn_bwd_f32:  t_i = Zn_i . dZn_i  (row kernel)
//             dY = rn (dZn - Zn t);  train mode: dgamma = sum_i dY xhat, dbeta = sum_i dY, dX = a (dY - dbeta / N - xhat dgamma / N)   (column kernel:
//             a workgroup per (episode, 32-feature slab) keeps the slab's dY in LDS between the two passes over the rows)
// The kernels live in dkt_frontend_big_kernels.h, templated on the element type of X / dX (fp32 here; bf16 / f16 in dkt_frontend_x16.hip).
#include "dkt_common.h"
#include "dkt_frontend_big_kernels.h"
#include "../../include/dkt_abi.h"

extern "C" int dkt_affine_normalize_f32(const float* X, const float* a, const float* s, long ab_bstride, float* Zn, float* rnorm, int B, int N, int D, void* stream) {
    if (!X || !a || !s || !Zn || !rnorm || B <= 0 || N <= 0 || D <= 0) return DKT_ERR_BAD_ARG;
    if ((D & 3) || ((uintptr_t)X & 15) || ((uintptr_t)Zn & 15) || ((uintptr_t)a & 15) || ((uintptr_t)s & 15) || (ab_bstride & 3) || ab_bstride < 0) return DKT_ERR_BAD_ARG;
    const long rows = (long)B * N;
    if ((rows + 3) / 4 > 0x7fffffffL) return DKT_ERR_TOO_LARGE;
    return affine_normalize_launch<float>(X, a, s, ab_bstride, Zn, rnorm, rows, N, D, (hipStream_t)stream);
}

extern "C" int dkt_normalize_bn_bwd_f32(const float* dZn, const float* Zn, const float* X, const float* a, long a_bstride, const float* mean, const float* rstd,
                                        const float* rnorm, float* dX, float* dgamma_part, float* dbeta_part, float* rowdot_ws, int B, int N, int D, void* stream) {
    if (!dZn || !Zn || !a || !rnorm || !dX || !rowdot_ws || B <= 0 || N <= 0 || D <= 0) return DKT_ERR_BAD_ARG;
    const bool train = mean != nullptr;
    if (train && (!X || !rstd || !dgamma_part || !dbeta_part)) return DKT_ERR_BAD_ARG;
    if ((D & 3) || ((uintptr_t)dZn & 15) || ((uintptr_t)Zn & 15) || ((uintptr_t)X & 15) || ((uintptr_t)dX & 15) || ((uintptr_t)a & 15) || (a_bstride & 3) || a_bstride < 0)
        return DKT_ERR_BAD_ARG;
    if (train && (((uintptr_t)mean & 15) || ((uintptr_t)rstd & 15) || ((uintptr_t)dgamma_part & 15) || ((uintptr_t)dbeta_part & 15))) return DKT_ERR_BAD_ARG;
    if (N > 1024) return DKT_ERR_TOO_LARGE;                                  // the slab's dY lives in LDS: 128 B per row
    const long rows = (long)B * N;
    const int nslab = (D + 31) / 32;
    if ((rows + 3) / 4 > 0x7fffffffL || (long)B * nslab > 0x7fffffffL) return DKT_ERR_TOO_LARGE;
    return normalize_bn_bwd_launch<float>(dZn, Zn, X, a, a_bstride, mean, rstd, rnorm, dX, dgamma_part, dbeta_part, rowdot_ws, B, N, D, train, (hipStream_t)stream);
}
