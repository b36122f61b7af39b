// dkt_mll_mfma.hip -- exact-GP marginal likelihood for N + 1 <= 128, ONE WAVE PER CLASS MATRIX, the whole
// factorisation / inversion / K^-1 product on v_mfma_f32_16x16x4_f32 with operands taken straight from accumulators.
//
// Replaces `-self.mll(output, targets)`, its autograd backward and the eval-mode mean cache
// (reference methods/DKT.py:161-163, 177, 187, 252-254, 265, 330; methods/DKT_regression.py:53-56, 92), i.e. GPyTorch's
// psd_safe_cholesky / inv_quad_logdet / cholesky_solve, for the C one-vs-rest models K_c = sv_c E + noise_c I of an episode.
//
// Workgroup = two episodes, one wave per class (C > 5: classes in rounds).  A wave keeps the upper block triangle of the
// (N+1)-augmented, 16-padded matrix
//        K' = [ K  r ; r^T 0 ] (+ identity on the padding),      r = y_c - m_c,
// as 16 x 16 tiles in the MFMA accumulator layout (lane (g, c), register q  <->  element [4g + q][c]; NT (NT+1) / 2 tiles,
// 4 VGPRs each).  The layout makes register q of a tile X a valid A operand (it is rows {q, q+4, q+8, q+12} of X,
// transposed) and register q of a tile Y a valid B operand (the same rows of Y), so
//        D += X^T Y   =   4 MFMAs, no LDS, no shuffles, no copies                                   (xty below)
// and every step of an UPPER (K' = R^T R) blocked algorithm is of that shape:
//   1. factorisation, block column k:  diagonal tile -> sweep (below) -> M_kk = R_kk^-T;   panel R_kj = (-V_kk)^T S_kj
//      (V_kk = M_kk^T through one X^T (-I) product);   trailing S_ij += R_ki^T R_kj.   Tiles hold S = -(Schur complement),
//      so the accumulate form of the MFMA is the update and no operand is ever negated.
//   2. inverse M = R^-T (lower), row j:  M_ji = (-V_jj)^T sum_{i<=k<j} R_kj^T M_ki, written over R_ij's slot.
//   3. K'^-1 = M^T M, in place:  P_ij = sum_{k>=j} M_ki^T M_kj.
// The augmented column does the vector work: column N of R is w = R^-T r, the Schur value met at pivot N is -|w|^2
// (the quadratic form), row N of M is -alpha^T, and with the sign of that row flipped in the A operand of step 3 the
// product is K^-1 - alpha alpha^T, i.e. -2 x the class's contribution to d logp / d K.  Pivot N and the padding pivots are
// forced to 1.
//
// Diagonal tile (the only VALU part, 16 pivots): the symmetric tile goes from the accumulator layout to a replicated
// column layout (every 16-lane row holds the whole tile, lane c = column c in 16 registers; v_permlane32_swap /
// v_permlane16_swap), where Gaussian elimination of [A | I] is one DPP-fused instruction per row and pivot:
//        a[i] += row_newbcast_p(a[i]) * (a[p] / -d),     b[i] += row_newbcast_p(a[i]) * (b[p] / -d)
// leaving d_p on the diagonal of a and, with rows scaled by 1/sqrt(d_p) as they become final, M_kk = R_kk^-T in b.
//
// W[b] = sum_c cls_weight_c sv_c 0.5 (alpha alpha^T - K_c^-1) is accumulated over the classes in LDS (tile layout, the
// waves take turns in a fixed order: deterministic) and stored ONCE, mirrored.  HBM traffic = E read + W written.
//
// This file: the fp32 arithmetic policy (ArithF32: the panel product and the Cholesky output), the kernel body and the launcher.  Tile indexing and
// forming, the pending-update schedule dealt over the sweep, the head of a factorisation step and E staging are shared with the f16-split successor
// (dkt_mll_h2.hip) and live once in dkt_wave_mll.h.
#include "dkt_wave_mll.h"

namespace {

using namespace dkt_mfma;

#ifndef DKT_MFMA_SWEEP_PRIO   // issue priority of a sweeping wave (sweep_prio, dkt_wave_mll.h)
#define DKT_MFMA_SWEEP_PRIO 1
#endif

struct P1F32 : P1Base {
    float* Lmat;             // CHOL: this matrix' L[N, N]
    float lsc;               // CHOL: sqrt(kappa), L = L_s sqrt(kappa)
    f32x4 negI;
    int N;
};

// exact fp32 on v_mfma_f32_16x16x4_f32: tiles hold S = -(Schur complement) as they are
template <bool CHOL>
struct ArithF32 {
    static constexpr float PAD_DIAG = -1.0f;
    static constexpr int NMFMA = 4;
    static constexpr int SWEEP_PRIO = DKT_MFMA_SWEEP_PRIO;
    static __device__ __forceinline__ f32x4 acc(const f32x4 x, const f32x4 y, const f32x4 c) { return xty(x, y, c); }
    template <int Q>
    static __device__ __forceinline__ f32x4 acc1(const f32x4 x, const f32x4 y, const f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(x[Q], y[Q], c, 0, 0, 0); }
    static __device__ __forceinline__ void sweep_begin(const f32x4 S, float (&x)[16], float& dv) { dkt_mfma::sweep_begin(S, x, dv); }

    template <int NT, int K>
    static __device__ __forceinline__ void panel(Tiles<NT>& T, P1F32& c, const f32x4 M, const float (&x)[16], const Lane& ln, const bool valid) {
        if constexpr (CHOL) {
            // L[16K + c][16K + i] = R_KK[i][c] = -x[i] (i < c), 1 / M_KK[c][c] on the diagonal, zero above it
            if (ln.g0 && valid) {
                float* Lrow = c.Lmat + (size_t)(16 * K + c.c16) * c.N + 16 * K;
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (16 * K + i < c.N) Lrow[i] = (i < c.c16) ? -x[i] * c.lsc : ((i == c.c16) ? c.lsc / x[i] : 0.f);
            }
        }
        if constexpr (K + 1 < NT) {
            const f32x4 nV = xty0(M, c.negI);                                        // M^T (-I) = -V_KK
#pragma unroll
            for (int j = K + 1; j < NT; ++j) T.t[K][j] = xty0(nV, T.t[K][j]);        // panel: R_Kj
        }
    }
};

template <int NT, bool GRAD, bool CHOL, bool WPG5>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64 * MAX_WPG * epw<NT>()), amdgpu_waves_per_eu(NT <= 7 ? 3 : 2, NT <= 7 ? 3 : 2)))
void mll_mfma_kernel(MllArgs a, const int wpg) {
    using A = ArithF32<CHOL>;
    constexpr int NTT = ntt(NT);
    constexpr int EPW = epw<NT>();
    // per episode: the E tiles (raw, shared by the class waves) -- and, once every wave is done with them, the exchange buffer of
    // the sum over the classes (5 waves x ceil(NTT / 5) tiles)
    __shared__ f32x4 stage_all[EPW][(GRAD && WPG5 ? 5 * ((NTT + 4) / 5) : NTT) * 64];
    __shared__ f32x4 mst[MAX_WPG * EPW][NT * 64];           // per wave: the diagonal tiles M_kk
    __shared__ f32x4 yst[MAX_WPG * EPW][NT * 4];            // per wave: the targets of its class

    const int tid = threadIdx.x;
    const int wall = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave in the workgroup
    const int epl = wall / wpg;                                  // episode within the workgroup
    const int w = wall - epl * wpg;                              // wave within the episode
    const int b = min(blockIdx.x * EPW + epl, a.B - 1);
    const bool ep_ok = blockIdx.x * EPW + epl < a.B;             // an odd tail: the surplus waves only keep the barriers company
    f32x4* const stage = stage_all[epl];
    f32x4* const myst = mst[wall];
    f32x4* const myys = yst[wall];
    const int C = a.C;
    const float qnan = __int_as_float(0x7fc00000);
    const int nrounds = (C + wpg - 1) / wpg;

#ifdef DKT_MFMA_CLOCKS
    unsigned long long clk[32] = {};
    unsigned long long clk2[16] = {};
#endif
    DKT_CLK(0);
    for (int round = 0; round < nrounds; ++round) {
        // lane coordinates and sizes made opaque per round: keeps the compiler from hoisting (and then spilling) every mask and
        // address of the round body into the kernel prologue
        int tq = tid;
        DKT_OPAQUE_V(tq);
        int c16 = tq & 15, g4 = (tq >> 2) & 12, lane = tq & 63, N = a.N;
        DKT_OPAQUE_S(N);
        Lane ln;
        ln.lane = lane; ln.g = g4 >> 2; ln.c = c16;
        ln.g0 = ln.g == 0; ln.g1 = ln.g == 1; ln.g2 = ln.g == 2;
        const int pN = N - 16 * (NT - 1);                        // local index of the augmented row / column in the last tile
        const int c = round * wpg + w;
        const bool active = ep_ok && c < C;
        // ---- stage E[b] (the waves of the episode share the loads) and this wave's targets ----
        if (ep_ok) {
            const brsrc Er = mk_rsrc(a.E + (size_t)b * N * N, (unsigned)(N * N * 4));
            stage_e<NT, 0, 0>(stage, Er, N, pN, c16, g4, lane, w, wpg);
        }
        if (active) {
            const brsrc yr = mk_rsrc(a.Y + (size_t)b * a.y_bstride + (size_t)c * N, (unsigned)(N * 4));
            float* ysf = reinterpret_cast<float*>(myys);
            if (lane < 16 * NT) ysf[lane] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(yr, lane * 4, 0, 0));     // beyond N: 0
            if (NT > 4 && lane + 64 < 16 * NT) ysf[lane + 64] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(yr, (lane + 64) * 4, 0, 0));
        }
        __syncthreads();
        DKT_CLK(1);
        Tiles<NT> T;
        float coef = 0.f;
        if (active) {
            f32x4 negI;
#pragma unroll
            for (int q = 0; q < 4; ++q) negI[q] = (g4 + q == c16) ? -1.0f : 0.0f;
            const float svc = a.sv[c], mc = a.mean[c], nzc = a.noise[c];
            const size_t bc = (size_t)b * C + c;
            FormCtxT<false> f;
            f.es = stage; f.ys = myys;
#ifdef DKT_MFMA_CLOCKS
            f.clk2 = clk2;
#endif
            f.pN = pN; f.c16 = c16; f.g4 = g4; f.lane = lane; f.mc = mc;
            // Scale by kappa = 4^m >= max_i K_ii (exact in fp32): every pivot of K / kappa is <= 1, which the sweep's update at the
            // pivot lane relies on.  With r / 2^m in the augmented column, w and the quadratic form are unchanged;
            // alpha = alpha_s / 2^m, K^-1 - alpha alpha^T = (.)_s / kappa, log det K = log det K_s + N log kappa.
            float emax = 0.f;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const f32x4 e = stage[tidx(j, j) * 64 + lane];
#pragma unroll
                for (int q = 0; q < 4; ++q) emax = fmaxf(emax, (g4 + q == c16) ? e[q] : 0.f);
            }
            emax = wave_reduce_dpp<true>(emax);
            int fail_at = 0;
            float jit = 0.f, lsum = 0.f, quad = 0.f;
            int msc = 0;
            for (int attempt = 0; attempt <= a.max_tries; ++attempt) {
                jit = dkt_jitter_rung(a.jitter0, attempt);
                int ex;
                (void)frexpf(fmaf(svc, emax, nzc + jit), &ex);                 // max K_ii = f 2^ex, 0.5 <= f < 1
                msc = max(0, (ex + 1) >> 1);
                const float ikap = ldexpf(1.0f, -2 * msc);                      // 1 / kappa
                f.nsv = -svc * ikap;
                f.dg = -(nzc + jit) * ikap;
                f.rsc = ldexpf(1.0f, -msc);
                form_row0<A, NT, 0>(T, f);
                // ---- phase 1: factorisation.  The sweep of tile k + 1 runs ahead, interleaved with step k's remaining updates ----
                P1F32 pc;
                pc.myst = myst; pc.Lmat = CHOL ? a.L + bc * N * N : nullptr; pc.lsc = ldexpf(1.0f, msc); pc.negI = negI;
                pc.lane = lane; pc.c16 = c16; pc.pN = pN; pc.N = N;
                pc.fail_at = 0; pc.lsum = 0.f; pc.quad = 0.f;
#ifdef DKT_MFMA_CLOCKS
                pc.clk = clk;
                clk[9] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));      // HW_REG_HW_ID, bits 0..31
                clk[12] = __builtin_amdgcn_s_memtime();
#endif
                {
                    float dv, x[16];
                    sweep_prio<A, true>();
                    A::sweep_begin(T.t[0][0], x, dv);
                    sweep_interleaved<A, NT, -1, 0, NT == 1>(T, f, x, dv, ln, pN);
                    sweep_prio<A, false>();
                    phase1_step<A, NT, 0>(T, f, pc, x, dv, ln);
                }
                fail_at = pc.fail_at; lsum = pc.lsum; quad = pc.quad;
                if (fail_at == 0) break;
            }
            DKT_CLK(2);
            if constexpr (CHOL) {
                // off-diagonal tiles: L[16j + c][16k + 4g + q] = R_kj[4g+q][c]; the strictly upper tiles of L are zero
                const brsrc Lr = mk_rsrc(a.L + bc * N * N, (unsigned)(N * N * 4));
#pragma unroll
                for (int j = 1; j < NT; ++j) {
                    const bool row_ok = (j < NT - 1) || (c16 < pN);
#pragma unroll
                    for (int k = 0; k < j; ++k) {
                        bstore4(Lr, T.t[k][j] * ldexpf(1.0f, msc), row_ok ? ((16 * j + c16) * N + 16 * k + g4) * 4 : OOB, 0);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const bool ok = (j < NT - 1) || (g4 + q < pN);
                            bstore1(Lr, 0.f, ok ? ((16 * k + c16) * N + 16 * j + g4 + q) * 4 : OOB, 0);
                        }
                    }
                }
            }
            // ---- phase 2: M = R^-T; M_ji (j > i) overwrites slot (i, j); two rows i at a time (independent MFMA chains) ----
            // (lane coordinates opaque again: what the later phases derive from them is recomputed here instead of being kept
            // alive -- spilled -- across the factorisation)
            tq = tid;
            DKT_OPAQUE_V(tq);
            c16 = tq & 15; g4 = (tq >> 2) & 12; lane = tq & 63;
            f32x4 negI2;
#pragma unroll
            for (int q = 0; q < 4; ++q) negI2[q] = (g4 + q == c16) ? -1.0f : 0.0f;
#pragma unroll
            for (int j = 1; j < NT; ++j) {
                __builtin_amdgcn_sched_barrier(0);
                const f32x4 nV = xty0(myst[j * 64 + lane], negI2);
#pragma unroll
                for (int i = 0; i < j; i += 2) {
                    if (i + 1 < j) {
                        f32x4 QA = xty0(T.t[i][j], myst[i * 64 + lane]);                 // k = i
                        f32x4 QB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int k = i + 1; k < j; ++k)
                            xty2(T.t[k][j], T.t[i][k], QA, T.t[k][j], (k == i + 1) ? myst[k * 64 + lane] : T.t[i + 1][k], QB);
                        f32x4 RA = {0.f, 0.f, 0.f, 0.f}, RB = {0.f, 0.f, 0.f, 0.f};
                        xty2(nV, QA, RA, nV, QB, RB);
                        T.t[i][j] = RA;
                        T.t[i + 1][j] = RB;
                    } else {
                        f32x4 Q = xty0(T.t[i][j], myst[i * 64 + lane]);
#pragma unroll
                        for (int k = i + 1; k < j; ++k) Q = xty(T.t[k][j], T.t[i][k], Q);
                        T.t[i][j] = xty0(nV, Q);
                    }
                }
            }
            DKT_CLK(3);
            // ---- alpha = -(row N of M) ----
            const bool arow = (ln.g == (pN >> 2));
            const int qn = pN & 3;
            float asum = 0.f;
            {
                const brsrc ar = mk_rsrc(a.alpha + bc * N, (unsigned)(N * 4));
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const f32x4 m = (i < NT - 1) ? T.t[i][NT - 1] : myst[(NT - 1) * 64 + lane];
                    const float v = -(qn == 0 ? m[0] : qn == 1 ? m[1] : qn == 2 ? m[2] : m[3]) * f.rsc;
                    const bool ok = arow && ((i < NT - 1) || (c16 < pN));
                    bstore1(ar, (fail_at != 0) ? qnan : v, ok ? (16 * i + c16) * 4 : OOB, 0);
                    asum += ok ? v : 0.f;
                }
            }
            float trpp = 0.f;
            DKT_CLK(4);
            if constexpr (GRAD) {
                // ---- phase 3: P''_ij = sum_{k >= j} flip(M_ki)^T M_kj, in place (flip: the sign of row N) ----
                f32x4 sgn;
#pragma unroll
                for (int q = 0; q < 4; ++q) sgn[q] = (g4 + q == pN) ? -1.0f : 1.0f;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    __builtin_amdgcn_sched_barrier(0);
                    // i = 0 .. j-1 in pairs, then the diagonal (whose LDS slot the others still read) last
#pragma unroll
                    for (int i = 0; i <= j; i += 2) {
                        const bool pair = i + 1 <= j;
                        f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accB = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int k = j; k < NT; ++k) {
                            const f32x4 Bm = (k == j) ? myst[k * 64 + lane] : T.t[j][k];
                            f32x4 A0 = (k == i) ? myst[k * 64 + lane] : T.t[i][k];
                            if (k == NT - 1) A0 = A0 * sgn;
                            if (pair) {
                                f32x4 A1 = (k == i + 1) ? myst[k * 64 + lane] : T.t[i + 1][k];
                                if (k == NT - 1) A1 = A1 * sgn;
                                xty2(A0, Bm, accA, A1, Bm, accB);
                            } else {
                                accA = xty(A0, Bm, accA);
                            }
                        }
                        auto put = [&](const f32x4 acc, const int ii) {
                            if (ii < j) {
                                T.t[ii][j] = acc;
                            } else {
                                // diagonal tile: M_jj is dead now, P''_jj takes its place in LDS; trace over the real rows
                                myst[j * 64 + lane] = acc;
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const bool ok = (g4 + q == c16) && ((j < NT - 1) || (c16 < pN));
                                    trpp += ok ? acc[q] : 0.f;
                                }
                            }
                        };
                        put(accA, i);
                        if (pair) put(accB, i + 1);
                    }
                }
            }
            DKT_CLK(5);
            lsum = wave_reduce_dpp<false>(lsum) + (float)(2 * msc * N);            // log2 det K = log2 det K_s + N log2 kappa
            trpp *= ldexpf(1.0f, -2 * msc);
            asum = wave_reduce_dpp<false>(asum);
            trpp = wave_reduce_dpp<false>(trpp);
            if (lane == 0) {
                const bool ok = fail_at == 0;
                // explicit fmas: left to -ffp-contract the compiler fused another product in the GRAD = false instantiation than in the GRAD = true one
                // (fma(c, lsum, -0.5 quad) there, fma(-0.5, quad, c lsum) here), and the forward-only call's logp was an ulp off the training call's
                a.logp[bc] = ok ? fmaf(-(float)N, DKT_HALF_LOG_2PI, fmaf(-0.5f, quad, -0.34657359027997264f * lsum)) : qnan;
                a.jitter_used[bc] = jit;
                a.info[bc] = fail_at;
                if constexpr (GRAD) {
                    const float nz_eff = a.noise[c] + jit;                          // (re-read: cheaper than keeping them across the phases)
                    a.dmean[bc] = ok ? asum : qnan;
                    a.dnoise[bc] = ok ? -0.5f * trpp : qnan;                                    // 0.5 (alpha.alpha - tr K^-1)
                    a.dsv[bc] = ok ? 0.5f * ((quad - (float)N) + nz_eff * trpp) / a.sv[c] : qnan;
                }
            }
            if constexpr (CHOL) {
                if (fail_at != 0) {
                    float* Lb = a.L + bc * N * N;
                    for (int idx = lane; idx < N * N; idx += 64) Lb[idx] = qnan;
                }
            }
            const float cw = a.cls_weight ? a.cls_weight[c] : 1.0f;
            coef = (fail_at == 0) ? -0.5f * cw * a.sv[c] * ldexpf(1.0f, -2 * msc) : qnan;   // W_c = coef P''_s   (a failed class poisons W[b])
        }
        DKT_CLK(6);
        if constexpr (GRAD) {
            // ---- W[b] = sum over the classes of coef_c P''_c.  The staged E is dead once every wave is past its factorisation
            // (the barrier); its LDS becomes the exchange buffer. ----
            __syncthreads();
            tq = tid;
            DKT_OPAQUE_V(tq);
            c16 = tq & 15; g4 = (tq >> 2) & 12; lane = tq & 63;
            DKT_OPAQUE_S(N);
            const int pNs = N - 16 * (NT - 1);
            const brsrc Wr = mk_rsrc(a.W + (size_t)b * N * N, (unsigned)(N * N * 4));
            // tile n -> W[b]: element [4g+q][c] of tile (i, j) and its mirror; later rounds add to what this very wave stored before
            auto store_tile = [&](f32x4 v, const int i, const int j) {
                const bool col_ok = (j < NT - 1) || (c16 < pNs);
                const int vo_m = col_ok ? ((16 * j + c16) * N + 16 * i + g4) * 4 : OOB;       // i < j <= NT-1: real columns
                int vo_d[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bool row_ok = (i < NT - 1) || (g4 + q < pNs);
                    vo_d[q] = (row_ok && col_ok) ? ((16 * i + g4 + q) * N + 16 * j + c16) * 4 : OOB;
                }
                if (round > 0) {
                    if (i < j) {
                        v += bload4(Wr, vo_m, 0);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(Wr, vo_d[q], 0, 0));
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) bstore1(Wr, v[q], vo_d[q], 0);
                if (i < j) bstore4(Wr, v, vo_m, 0);
            };
            if constexpr (WPG5) {
                // Five chunks (tile n -> chunk n % 5).  Per chunk every wave drops its <= 6 scaled tiles into its own slots of the
                // exchange buffer (compile-time register tiles, no divergent access to them); after the barrier wave w sums the
                // five copies of tile 5 w + chunk (wave 0 also of tile 25 + chunk) in class order -- deterministic -- and stores it.
                constexpr int KMAX = (NTT + 4) / 5;
#pragma unroll
                for (int g = 0; g < 5; ++g) {
                    if (ep_ok) {
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
#pragma unroll
                            for (int i = 0; i <= j; ++i) {
                                const int n = tidx(i, j);
                                if (n % 5 != g) continue;
                                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                                if (active) v = ((i < j) ? T.t[i][j] : myst[j * 64 + lane]) * coef;
                                stage[(w * KMAX + n / 5) * 64 + lane] = v;
                            }
                        }
                    }
                    __syncthreads();
                    if (ep_ok) {
                        for (int k = w; 5 * k + g < NTT; k += 5) {
                            f32x4 v = stage[k * 64 + lane];
#pragma unroll
                            for (int ww = 1; ww < 5; ++ww) v += stage[(ww * KMAX + k) * 64 + lane];
                            const int n = 5 * k + g;
                            int j = 0;
                            while ((j + 1) * (j + 2) / 2 <= n) ++j;          // wave-uniform: tile n = (i, j), i <= j
                            store_tile(v, n - j * (j + 1) / 2, j);
                        }
                    }
                    if (g < 4 || round + 1 < nrounds) __syncthreads();
                }
            } else {
                // general class count per round: the waves take turns adding all their tiles (fixed order), then share the stores
                for (int t = 0; t < wpg; ++t) {
                    if (t == w && active) {
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
#pragma unroll
                            for (int i = 0; i <= j; ++i) {
                                f32x4 v = ((i < j) ? T.t[i][j] : myst[j * 64 + lane]) * coef;
                                f32x4* p = &stage[tidx(i, j) * 64 + lane];
                                if (t > 0) v += *p;
                                *p = v;
                            }
                        }
                    }
                    __syncthreads();
                }
                if (ep_ok) {
                    for (int n = w; n < NTT; n += wpg) {
                        int j = 0;
                        while ((j + 1) * (j + 2) / 2 <= n) ++j;
                        store_tile(stage[n * 64 + lane], n - j * (j + 1) / 2, j);
                    }
                }
                if (round + 1 < nrounds) __syncthreads();
            }
        } else {
            if (round + 1 < nrounds) __syncthreads();            // the next round re-stages E
        }
    }
    DKT_CLK(7);
#ifdef DKT_MFMA_CLOCKS
    DKT_CLK(8);
    if ((tid & 63) == 0 && a.ws) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(a.ws) + ((size_t)blockIdx.x * (MAX_WPG * EPW) + wall) * 48;
        for (int i = 0; i < 32; ++i) o[i] = clk[i];
        for (int i = 0; i < 16; ++i) o[32 + i] = clk2[i];
    }
#endif
}

template <int NT>
void launch_mfma(const MllArgs& a, hipStream_t st) {
    const bool g = (a.flags & DKT_MLL_WANT_GRAD) != 0, c = (a.flags & DKT_MLL_WANT_CHOL) != 0;
    const int rounds = (a.C + MAX_WPG - 1) / MAX_WPG;
    const int wpg = (a.C + rounds - 1) / rounds;
    constexpr int EPW = epw<NT>();
    const dim3 grid((a.B + EPW - 1) / EPW), block(64 * wpg * EPW);
    if (g && c && wpg == 5) { hipLaunchKernelGGL((mll_mfma_kernel<NT, true, true, true>), grid, block, 0, st, a, wpg); return; }
    if (g && c) { hipLaunchKernelGGL((mll_mfma_kernel<NT, true, true, false>), grid, block, 0, st, a, wpg); return; }
    if (c) { hipLaunchKernelGGL((mll_mfma_kernel<NT, false, true, false>), grid, block, 0, st, a, wpg); return; }
#ifdef DKT_TWINS         // without the Cholesky output this kernel is the exact-fp32 twin of dkt_mll_h2.hip (DKT_MLL_FORCE_F32MFMA)
    if (g && wpg == 5) hipLaunchKernelGGL((mll_mfma_kernel<NT, true, false, true>), grid, block, 0, st, a, wpg);
    else if (g) hipLaunchKernelGGL((mll_mfma_kernel<NT, true, false, false>), grid, block, 0, st, a, wpg);
    else hipLaunchKernelGGL((mll_mfma_kernel<NT, false, false, false>), grid, block, 0, st, a, wpg);
#endif
}

}  // namespace

// The product library serves DKT_MLL_WANT_CHOL here for N + 1 <= 32 (the regression head's conditioning sets, DKT_regression.py:84-93: 5 .. 19 rows; larger
// requests take the generic kernel) and nothing else; the twins library (-DDKT_TWINS) has every size with and without the Cholesky output -- the exact-fp32
// twin of the f16-split kernels.  This predicate is the one place that knows the difference (the switch below only instantiates what it admits).
bool dkt_mll_mfma_serves(int N, unsigned flags) {
#ifndef DKT_TWINS
    if (!(flags & DKT_MLL_WANT_CHOL) || N + 1 > 32) return false;
#endif
    return N + 1 <= 128;
}
void dkt_mll_mfma_launch(const MllArgs& a, hipStream_t st) {
    switch ((a.N + 1 + 15) / 16) {
        case 1: launch_mfma<1>(a, st); break;
        case 2: launch_mfma<2>(a, st); break;
#ifdef DKT_TWINS
        case 3: launch_mfma<3>(a, st); break;
        case 4: launch_mfma<4>(a, st); break;
        case 5: launch_mfma<5>(a, st); break;
        case 6: launch_mfma<6>(a, st); break;
        case 7: launch_mfma<7>(a, st); break;
        case 8: launch_mfma<8>(a, st); break;
#endif
        default: break;                                    // unreachable: mll_plan() sends only what dkt_mll_mfma_serves()
    }
}
