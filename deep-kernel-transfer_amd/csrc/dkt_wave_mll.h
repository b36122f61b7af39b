// dkt_wave_mll.h -- the ONE-WAVE-PER-CLASS-MATRIX skeleton of the marginal-likelihood kernels for N + 1 <= 128, shared by the exact-fp32
// kernel (dkt_mll_mfma.hip: mll_mfma_kernel) and its f16-split successors (dkt_mll_h2.hip: mll_h2_kernel, and through FormCtxT<true>
// the wave-per-episode mll_h2e_kernel).  The algorithm is described in the header of dkt_mll_mfma.hip, the f16 scales in that of
// dkt_mll_h2.hip.  Here, once: the tile indexing, forming K' from the staged E, the pending-update schedule that deals block step K's
// trailing MFMAs over the sweep of diagonal tile K + 1, the head of a factorisation step, E staging and loading, the measurement
// build's clock hooks.  The kernel BODIES (round preamble, jitter ladder, phases 2 and 3, the sum over the classes) are still spelled
// out in each .hip file: moved into functions of this header they compile to other register allocations (docs/MEASUREMENTS.md R19).
//
// What differs between the kernels is an ARITHMETIC POLICY `A`, a struct of the .hip file with
//   PAD_DIAG            the padding diagonal of the formed tiles (-1, or -2^30 where the accumulators hold 2^30 S)
//   NMFMA               single MFMAs per tile product (4 fp32, 3 f16 plane products)
//   SWEEP_PRIO          issue priority of a wave while it sweeps a diagonal tile (0 = off)
//   acc(x, y, c)        c + x^T y, a whole tile product;   acc1<Q>(x, y, c): one of its NMFMA instructions
//   sweep_begin(S, x, dv)   accumulator layout -> replicated column layout
//   panel<NT, K>(T, c, M, x, ln, valid)   what follows a swept diagonal tile: the Cholesky output (fp32 only) and the panel R_Kj, j > K
#pragma once
#include "dkt_h2_tiles.h"

namespace dkt_mfma {

#ifdef DKT_MFMA_CLOCKS      // measurement build (tools/mll_phase_clocks.py): s_memtime stamps per wave into the workspace pointer
#define DKT_CLK(i) do { __builtin_amdgcn_sched_barrier(0); clk[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define DKT_CLK(i) do { } while (0)
#endif
#define DKT_OPAQUE_V(x) asm volatile("" : "+v"(x))
#define DKT_OPAQUE_S(x) asm volatile("" : "+s"(x))

constexpr int ntt(int nt) { return nt * (nt + 1) / 2; }
__host__ __device__ constexpr int tidx(int i, int j) { return j * (j + 1) / 2 + i; }      // i <= j (the order the tile loops enumerate)

constexpr int MAX_WPG = 5;   // waves (classes) per episode and round

// Episodes per workgroup.  The dispatcher deals the waves of a workgroup to the 4 SIMDs round-robin from SIMD 0, and at 3 waves per
// SIMD (168 VGPRs) a second 5-wave workgroup no longer fits on SIMD 0: measured one resident workgroup per CU.  Two episodes = 10
// waves per workgroup load the SIMDs (3, 3, 2, 2).  NT = 8 runs at 2 waves per SIMD (256 VGPRs): one episode per workgroup.
template <int NT> constexpr int epw() { return NT <= 7 ? 2 : 1; }

template <int NT>
struct Tiles {
    f32x4 t[NT][NT];         // [i][j], i < j: off-diagonal slots;  [j][j]: diagonal slot
};

// Issue priority of a wave while it sweeps a diagonal tile (VALU work that competes for the shared fp32-MFMA / VALU pipe with the
// matrix instructions of the other waves of the SIMD): s_setprio.  0 = off.  Measured: -2 % (N = 105) / -3.5 % (N = 85) at 1; 3, or the
// whole factorisation at 1, are no different.
template <class A, bool ON>
__device__ __forceinline__ void sweep_prio() {
    if constexpr (A::SWEEP_PRIO != 0) __builtin_amdgcn_s_setprio(ON ? A::SWEEP_PRIO : 0);
}

template <bool ER>
struct FormCtxT {
    static constexpr bool er = ER;   // true: the raw E tile sits in the tile's own register slot (wave-per-episode kernel); false: staged in LDS
    const f32x4* es;         // LDS: the episode's E tiles (raw, accumulator layout), shared by the waves of the episode
    const f32x4* ys;         // LDS: this wave's targets y_c, 16-byte groups
    int pN, c16, g4, lane;
    float nsv, dg, mc, rsc;  // -sv / kappa, -(noise + jitter) / kappa, mean, 1 / sqrt(kappa)  (f16: the first two and the last x 2^30, the last x rho)
#ifdef DKT_MFMA_CLOCKS
    unsigned long long* clk2;
#endif
};

// Tile (I, J), I <= J, of S = -K' (f16: 2^30 S) in the accumulator layout, from the staged E tile.  The last block column carries the
// augmented column -r (f16: -rho r_s; lanes c == pN), the last diagonal tile also its mirror row, a zero at the augmented pivot and
// -1 (A::PAD_DIAG) on the padding diagonal.
template <class A, int NT, int I, int J, class F>
__device__ __forceinline__ f32x4 form_tile(const Tiles<NT>& T, const F& f) {
    const int pN = f.pN, c16 = f.c16, g4 = f.g4;
    f32x4 e;
    if constexpr (F::er) e = T.t[I][J];
    else e = f.es[tidx(I, J) * 64 + f.lane];
    f32x4 s;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v = f.nsv * e[q];
        if (I == J) v = (g4 + q == c16) ? v + f.dg : v;
        s[q] = v;
    }
    if constexpr (J == NT - 1) {
        const f32x4 yv = f.ys[4 * I + (g4 >> 2)];                             // y[16 I + 4g + q]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool rok = (I < NT - 1) || (g4 + q < pN);
            s[q] = (c16 == pN) ? (rok ? (f.mc - yv[q]) * f.rsc : 0.f) : s[q];
        }
        if constexpr (I == NT - 1) {
            const float yc = reinterpret_cast<const float*>(f.ys)[16 * I + c16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = s[q];
                v = (g4 + q == pN) ? ((c16 < pN) ? (f.mc - yc) * f.rsc : 0.f) : v;   // mirror row of the augmented column; pivot N = 0
                v = (g4 + q > pN) ? ((g4 + q == c16) ? A::PAD_DIAG : 0.f) : v;  // padding: identity
                s[q] = v;
            }
        }
    }
    return s;
}

template <class A, int NT, int J, class F>
__device__ __forceinline__ void form_row0(Tiles<NT>& T, const F& f) {      // tiles (0, J), J = 0 .. NT-1
    if constexpr (J < NT) {
        T.t[0][J] = form_tile<A, NT, 0, J>(T, f);
        form_row0<A, NT, J + 1>(T, f);
    }
}

// tile row 1 of block step 0's trailing update, the freshly formed tiles as C operands: S_1j = form(1, j) + R_01^T R_0j
// (f16: 2^30 S_1j = form(1, j) + (2^15 R_01)^T (2^15 R_0j))
template <class A, int NT, int J, class F>
__device__ __forceinline__ void form_trailing_row1(Tiles<NT>& T, const F& f) {
    if constexpr (J < NT) {
        T.t[1][J] = A::acc(T.t[0][1], T.t[0][J], form_tile<A, NT, 1, J>(T, f));
        form_trailing_row1<A, NT, J + 1>(T, f);
    }
}

// Trailing updates of block step K that are NOT needed by the next sweep (tile rows i >= K + 2), u = 0 .. n_pending - 1 in (i, j) order.
template <int NT, int K> constexpr int n_pending() { return (K >= 0 && NT - K - 2 > 0) ? (NT - K - 2) * (NT - K - 1) / 2 : 0; }
template <int NT, int K> constexpr int pend_i(int u) { int i = K + 2; while (u >= NT - i) { u -= NT - i; ++i; } return i; }
template <int NT, int K> constexpr int pend_j(int u) { int i = K + 2; while (u >= NT - i) { u -= NT - i; ++i; } return i + u; }

// The pending updates as a stream of single MFMAs, S = 0 .. n_pend_mfma - 1, ordered so that neighbours belong to different tiles
// (two tile updates advance alternately, A::NMFMA instructions each: the dependent-accumulate latency of one hides behind the other).
template <class A, int NT, int K> constexpr int n_pend_mfma() { return 2 * A::NMFMA * ((n_pending<NT, K>() + 1) / 2); }

template <class A, int NT, int K, int S0, int S1, class F>
__device__ __forceinline__ void pend_mfma(Tiles<NT>& T, const F& f) {
    if constexpr (S0 < S1) {
        constexpr int PER = 2 * A::NMFMA;
        constexpr int u = 2 * (S0 / PER) + (S0 & 1), q = (S0 % PER) >> 1;
        if constexpr (u < n_pending<NT, K>()) {
            constexpr int i = pend_i<NT, K>(u), j = pend_j<NT, K>(u);
            if constexpr (K == 0 && q == 0) T.t[i][j] = form_tile<A, NT, i, j>(T, f);              // block step 0 consumes E as it goes
            T.t[i][j] = A::template acc1<q>(T.t[K][i], T.t[K][j], T.t[i][j]);
        }
        pend_mfma<A, NT, K, S0 + 1, S1>(T, f);
    }
}

// Slots of the sweep into which the pending MFMAs are dealt: one after every pivot's scalar chain and one after every piece of
// <= 5 row updates, i.e. about one MFMA (32 cycles of the matrix pipe) per 5-6 VALU instructions (~32 cycles of issue from one wave).
constexpr int slots_of_pivot(int p) { return 1 + (15 - p + 4) / 5; }
constexpr int slots_before(int p) { int n = 0; for (int i = 0; i < p; ++i) n += slots_of_pivot(i); return n; }
constexpr int SWEEP_SLOTS = slots_before(16);

template <class A, int NT, int K, int SLOT, class F>
__device__ __forceinline__ void run_slot(Tiles<NT>& T, const F& f) {
    constexpr int NM = n_pend_mfma<A, NT, K>();
    if constexpr (NM > 0) {
        pend_mfma<A, NT, K, SLOT * NM / SWEEP_SLOTS, (SLOT + 1) * NM / SWEEP_SLOTS>(T, f);
        __builtin_amdgcn_sched_barrier(0);                    // pin the MFMA between the VALU pieces
    }
}

template <class A, int NT, int K, int P, int I0, int SLOT, class F>
__device__ __forceinline__ void sweep_rows_slots(Tiles<NT>& T, const F& f, float (&x)[16], const float t) {
    if constexpr (I0 < 16) {
        constexpr int CNT = (16 - I0) < 5 ? (16 - I0) : 5;
        sweep_rows_piece<P, I0, CNT>(x, t);
        run_slot<A, NT, K, SLOT>(T, f);
        sweep_rows_slots<A, NT, K, P, I0 + CNT, SLOT + 1>(T, f, x, t);
    }
}

// The sweep of diagonal tile K + 1 with block step K's remaining trailing updates dealt over it: their MFMAs run on the matrix
// pipe underneath the sweep's VALU work of the same wave (K = -1: the very first tile, nothing pending).
template <class A, int NT, int K, int P, bool LAST, class F>
__device__ __forceinline__ void sweep_interleaved(Tiles<NT>& T, const F& f, float (&x)[16], float& dv, const Lane& ln, const int pn) {
    if constexpr (P < 16) {
        const float t = sweep_pivot_head<P, LAST>(x, dv, ln, pn);
#ifdef DKT_MFMA_CLOCKS
        if constexpr (K == -1) { __builtin_amdgcn_sched_barrier(0); f.clk2[P] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
#endif
        run_slot<A, NT, K, slots_before(P)>(T, f);
        sweep_rows_slots<A, NT, K, P, P + 1, slots_before(P) + 1>(T, f, x, t);
        sweep_interleaved<A, NT, K, P + 1, LAST>(T, f, x, dv, ln, pn);
    }
}

// What a factorisation carries from step to step; a policy's panel step derives its own context from it (its -I operand, the Cholesky output).
struct P1Base {
#ifdef DKT_MFMA_CLOCKS
    unsigned long long* clk;
#endif
    f32x4* myst;             // LDS: this wave's diagonal tiles M_kk (unused where they stay in the diagonal register slots)
    int lane, c16, pN;
    int fail_at;
    float lsum, quad;
};

// Block step K of the factorisation; x / dv hold the swept diagonal tile K on entry.
template <class A, int NT, int K, class F, class P1>
__device__ __forceinline__ void phase1_step(Tiles<NT>& T, const F& f, P1& c, float (&x)[16], float& dv, const Lane& ln) {
    if constexpr (K < NT) {
#ifdef DKT_MFMA_CLOCKS
        __builtin_amdgcn_sched_barrier(0);
        c.clk[13 + 2 * K] = __builtin_amdgcn_s_memtime();          // sweep K done
        __builtin_amdgcn_sched_barrier(0);
#endif
        const f32x4 M = sweep_end(x, ln);
        const bool valid = (K < NT - 1) || (c.c16 < c.pN);
        const unsigned long long badm = __ballot(valid && !(dv > 0.f)) & 0xffffull;
        const int first = (int)__builtin_ctzll(badm | 0x10000ull);
        c.fail_at = (c.fail_at == 0 && badm != 0) ? 16 * K + first + 1 : c.fail_at;
        c.lsum += (valid && ln.g0) ? __builtin_amdgcn_logf(dv) : 0.f;              // log2
        if constexpr (K == NT - 1) c.quad = -__int_as_float(__builtin_amdgcn_readlane(__float_as_int(dv), c.pN));
        if constexpr (F::er) T.t[K][K] = M;                     // wave-per-episode kernel: M_KK takes the (dead) diagonal slot
        else c.myst[K * 64 + c.lane] = M;
        A::template panel<NT, K>(T, c, M, x, ln, valid);
        if constexpr (K + 1 < NT) {
            // tile row K + 1 first: the next sweep and the next panel need it
            if constexpr (K == 0) form_trailing_row1<A, NT, 1>(T, f);
            else {
#pragma unroll
                for (int j = K + 1; j < NT; ++j) T.t[K + 1][j] = A::acc(T.t[K][K + 1], T.t[K][j], T.t[K + 1][j]);
            }
            __builtin_amdgcn_sched_barrier(0);
#ifdef DKT_MFMA_CLOCKS
            c.clk[14 + 2 * K] = __builtin_amdgcn_s_memtime();      // panel + tile row K + 1 issued
            __builtin_amdgcn_sched_barrier(0);
#endif
            sweep_prio<A, true>();
            A::sweep_begin(T.t[K + 1][K + 1], x, dv);
            sweep_interleaved<A, NT, K, 0, K + 1 == NT - 1>(T, f, x, dv, ln, c.pN);
            sweep_prio<A, false>();
            phase1_step<A, NT, K + 1>(T, f, c, x, dv, ln);
        }
    }
}

// E[b] tile (I, J) (raw) for the stage: E is symmetric, so element [4g+q][c] = E[16J + c][16I + 4g + q] -- one 16-byte load per
// lane; rows / columns beyond N read as 0.
template <int NT, int I, int J>
__device__ __forceinline__ f32x4 load_e_tile(const brsrc Er, const int N, const int pN, const int c16, const int g4) {
    const int row = 16 * J + c16;
    const bool row_ok = (J < NT - 1) || (c16 < pN);
    f32x4 e;
    if constexpr (I < NT - 1) {
        e = bload4(Er, row_ok ? (row * N + g4) * 4 : OOB, 16 * I * 4);
    } else {
        // last diagonal tile: the four columns may run past N (and past the end of E[b]): element-wise loads
#pragma unroll
        for (int q = 0; q < 4; ++q)
            e[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(Er, (row_ok && g4 + q < pN) ? (row * N + g4 + q) * 4 : OOB, 16 * I * 4, 0));
    }
    return e;
}

template <int NT, int I, int J>
__device__ __forceinline__ void stage_e(f32x4* es, const brsrc Er, const int N, const int pN, const int c16, const int g4, const int lane,
                                        const int w, const int wpg) {
    if constexpr (J < NT) {
        if ((tidx(I, J) % wpg) == w) es[tidx(I, J) * 64 + lane] = load_e_tile<NT, I, J>(Er, N, pN, c16, g4);
        if constexpr (I < J) stage_e<NT, I + 1, J>(es, Er, N, pN, c16, g4, lane, w, wpg);
        else stage_e<NT, 0, J + 1>(es, Er, N, pN, c16, g4, lane, w, wpg);
    }
}

// E[b] -> the tile registers, diagonal tiles first (wave-per-episode kernel)
template <int NT, int J>
__device__ __forceinline__ void load_e_diag(Tiles<NT>& T, const brsrc Er, const int N, const int pN, const int c16, const int g4) {
    if constexpr (J < NT) {
        T.t[J][J] = load_e_tile<NT, J, J>(Er, N, pN, c16, g4);
        load_e_diag<NT, J + 1>(T, Er, N, pN, c16, g4);
    }
}
template <int NT, int I, int J>
__device__ __forceinline__ void load_e_off(Tiles<NT>& T, const brsrc Er, const int N, const int pN, const int c16, const int g4) {
    if constexpr (I < NT - 1) {
        if constexpr (J < NT) {
            T.t[I][J] = load_e_tile<NT, I, J>(Er, N, pN, c16, g4);
            load_e_off<NT, I, J + 1>(T, Er, N, pN, c16, g4);
        } else {
            load_e_off<NT, I + 1, I + 2>(T, Er, N, pN, c16, g4);
        }
    }
}
template <int NT>
__device__ __forceinline__ void load_all_e(Tiles<NT>& T, const brsrc Er, const int N, const int pN, const int c16, const int g4) {
    load_e_diag<NT, 0>(T, Er, N, pN, c16, g4);
    load_e_off<NT, 0, 1>(T, Er, N, pN, c16, g4);                 // row-major over the upper triangle: the order the factorisation consumes them
}

}  // namespace dkt_mfma
