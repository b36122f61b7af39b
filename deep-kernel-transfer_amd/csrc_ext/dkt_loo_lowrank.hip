// libdkt_loofs.so (include/dkt_abi_loofs.h; docs/LOOFS.md): the leave-one-out predictive log likelihood of B x C exact-GP problems
// K = sv_c Z Z^T + (noise_c + jitter) I for the linear kernels in FEATURE space, its N leave-one-out predictions and its gradients, in ONE launch.
// No N x N matrix exists: with s = noise + jitter, lam = s / sv, A = Z^T Z + lam I [D,D] and G = A^-1,
//     (K^-1 r)_i = (r_i - z_i.G Z^T r) / s,   (K^-1)_ii = (1 - z_i^T G z_i) / s.
//
// ONE kernel instance, 256 threads, plain fp32 on the VALU, a workgroup per EPISODE: Z is streamed in blocks of kR = 64 rows (an episode of 420 x 64 is
// 105 KiB, and N is unbounded), every D x D matrix is a 64 x 64 one in LDS (features past D are zero), every product runs in 4 x 4 register tiles.
//   pass 1   S = Z^T Z and the column sums of Z, once per episode: S to the workspace (both triangles), from where every rung of every class stages A.
//   then the C class models one after the other --
//   p = Z^T r straight from global memory (four interleaved row groups, summed in pairs);
//   the jitter ladder of dkt_loo_f32 on A (the factor-and-invert family of csrc/dkt_lds_dense.h): L, t = L^-1 p carried along as row D, U = L^-T,
//   w = U t, G = U U^T mirrored into a dense matrix;
//   pass 2   per block T = Z_blk G -> h_i, z_i.w (16 lanes per row group, xor butterflies) -> alpha, mu_loo, var_loo, the terms of loo and of the
//            hyper-parameter sums; with the gradient Z^T a and M = Z^T diag(c) Z (a second 4 x 4 tile per thread, the blocks in index order);
//   Q = -G (M + 1/2 (gw p^T + p gw^T)) G, two 64^3 products through LDS, tr Q;
//   pass 3   per block dZ_blk (+)= cls_weight_c (2 diag(c) Z_blk G + 2 Z_blk Q - (a / s) w^T + r gp^T): the thread that owns an element of dZ[b] adds the
//            classes to it in index order (its own earlier write: no atomics, a fixed order).
// Everything of a row is derived from alpha_i and var_i = s / (1 - h_i): a_i = -alpha_i var_i, b_i = (var_i + a_i^2) / 2, c_i = -b_i / s; pass 3 reads
// the two back from the outputs.  Every reduction has a fixed order that depends on nothing but (N, D).
#include "../../include/dkt_abi_loofs.h"
#include "dkt_lds_dense.h"

namespace {

using namespace dkt_lds;                 // the factor-and-invert family of dkt_lds_dense.h, kWave, wave_sum, kHalfLog2Pi, set_lds
constexpr int kT = 256;
constexpr int kDP = DKT_LOOFS_MAX_D;     // features, zero-padded to it
constexpr int kR = DKT_LOOFS_ROWS;       // rows of Z a workgroup holds at a time
constexpr int kLd = kDP + 4;             // row stride of the dense matrices and of the block of Z: float4 along a row, scalars down a column
constexpr int kDPP = kDP | 1;            // row stride of the factor (= padded(kDP))
constexpr int kMat = kDP * kLd;          // floats per matrix
constexpr int kVecs = 21;                // sd .. sred below, kDP floats each
static_assert(kDP == 64 && kR == 64 && kT == 256, "the 4 x 4 register tiles below cover 64 x 64 with 256 threads");
static_assert((kDP + 1) * kDPP <= kMat, "the factor and its right-hand side fit the matrix M takes over");

inline size_t loofs_lds_bytes() { return ((size_t)4 * kMat + kVecs * kDP) * sizeof(float); }

struct LoofsArgs {
    const float *Z, *Y, *sv, *mean, *noise, *cw;
    float *loo, *alpha, *mu, *var, *dZ, *dsv, *dmean, *dnoise, *jit, *S;
    int32_t* info;
    long ybs;
    int C, N, D, max_tries;
    float jitter0;
    unsigned flags;
};

// rows i0 .. i0 + kR - 1 of Z [N, D] -> dst (rows of kLd floats), rows past N and features past D zero
__device__ __forceinline__ void stage_rows(float* dst, const float* __restrict__ Zp, int i0, int N, int D, int tid) {
    const int ty = tid >> 4, c4 = (tid & 15) * 4;
#pragma unroll 1
    for (int it = 0; it < kR / 16; ++it) {
        const int r = it * 16 + ty;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 + r < N && c4 < D) v = *reinterpret_cast<const float4*>(Zp + (long)(i0 + r) * D + c4);
        *reinterpret_cast<float4*>(dst + r * kLd + c4) = v;
    }
}

// acc[i][j] += sum_{r < K} [sc_r] L[r][4 ty + i] R[r][4 tx + j]: the tile of L^T diag(sc) R, the terms in index order
template <bool SCALED>
__device__ __forceinline__ void tile_atb(float (&acc)[4][4], const float* L, const float* R, const float* sc, int K, int ty, int tx) {
#pragma unroll 2
    for (int r = 0; r < K; ++r) {
        const float4 la = *reinterpret_cast<const float4*>(L + r * kLd + 4 * ty);
        const float4 rb = *reinterpret_cast<const float4*>(R + r * kLd + 4 * tx);
        const float w = SCALED ? sc[r] : 1.f;
        const float a[4] = {SCALED ? w * la.x : la.x, SCALED ? w * la.y : la.y, SCALED ? w * la.z : la.z, SCALED ? w * la.w : la.w};
        const float bb[4] = {rb.x, rb.y, rb.z, rb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * bb[j];
    }
}

// acc[i][j] += sum_{k < K} Zs[4 ty + i][k] R[k][4 tx + j]: the tile of Z_blk R
__device__ __forceinline__ void tile_ab(float (&acc)[4][4], const float* Zs, const float* R, int K, int ty, int tx) {
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
        const float4 rb = *reinterpret_cast<const float4*>(R + k * kLd + 4 * tx);
        const float bb[4] = {rb.x, rb.y, rb.z, rb.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float z = Zs[(4 * ty + i) * kLd + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += z * bb[j];
        }
    }
}

// the sum over the 16 lanes of a row group (tx = 0 .. 15, neighbouring lanes), the same value in each
__device__ __forceinline__ float group_sum16(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__global__ __launch_bounds__(kT) void loofs_kernel(LoofsArgs a) {
    extern __shared__ float lds[];
    const int N = a.N, D = a.D, C = a.C;
    float* sG = lds;                     // G = A^-1, dense, zero past D
    float* sZ = sG + kMat;               // a block of Z
    float* sQ = sZ + kMat;               // M G, then Q
    float* sA = sQ + kMat;               // A (lower) + p (row D) -> L + t -> U -> G (lower); once G is mirrored: M + 1/2 (gw p^T + p gw^T)
    float* sM = sA;
    float* sd = sA + kMat;               // pivots of L
    float* st = sd + kDP;                // t = L^-1 p
    float* sw = st + kDP;                // w = G p
    float* sr = sw + kDP;                // diag G
    float* sp = sr + kDP;                // p = Z^T r
    float* sgw = sp + kDP;               // gw
    float* sgp = sgw + kDP;              // gp = G gw
    float* szs = sgp + kDP;              // the column sums of Z
    float* sa_ = szs + kDP;              // a_i of the block
    float* sc_ = sa_ + kDP;              // c_i of the block
    float* sx0 = sc_ + kDP;              // pass 3: 2 c_i
    float* sx1 = sx0 + kDP;              // ... -a_i / s
    float* sx2 = sx1 + kDP;              // ... r_i
    float* sterm = sx2 + kDP;            // the row terms of loo, sum a, sum (a alpha + b k)   [3][kDP]
    float* spart = sterm + 3 * kDP;      // the four partial sums of p                            [4][kDP]
    float* sred = spart + 4 * kDP;       // diag Q
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int ty = tid >> 4, tx = tid & 15;
    const bool grad = a.flags & DKT_LOOFS_WANT_GRAD;
    const float nan = __builtin_nanf("");
    const int b = blockIdx.x;
    const float* Zp = a.Z + (long)b * N * D;
    float* Sg = a.S + (long)b * kDP * kDP;
    float* dZp = grad ? a.dZ + (long)b * N * D : nullptr;

    // ---- pass 1: S = Z^T Z (a 4 x 4 tile per thread, both triangles) and the column sums, the rows in index order
    {
        float acc[4][4] = {};
        float zs = 0.f;
        for (int i0 = 0; i0 < N; i0 += kR) {
            stage_rows(sZ, Zp, i0, N, D, tid);
            __syncthreads();
            const int rows = min(kR, N - i0);
            tile_atb<false>(acc, sZ, sZ, nullptr, rows, ty, tx);
            if (tid < kDP)
                for (int r = 0; r < rows; ++r) zs += sZ[r * kLd + tid];
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<float4*>(Sg + (4 * ty + i) * kDP + 4 * tx) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        if (tid < kDP) szs[tid] = zs;
    }

    bool anybad = false;
    for (int c = 0; c < C; ++c) {
        const long prob = (long)b * C + c;
        const float* Yp = a.Y + (long)b * a.ybs + (long)c * N;
        const float v = a.sv[c], mu = a.mean[c], nz = a.noise[c];
        const float wc = a.cw ? a.cw[c] : 1.f;
        float* alp = a.alpha + prob * N;
        float* mup = a.mu + prob * N;
        float* varp = a.var + prob * N;

        // ---- p = Z^T r: column tid & 63, the rows g, g + 4, ... of group g = tid >> 6, the four groups summed in pairs
        __syncthreads();                           // (S of pass 1; the reads of the class before)
        {
            const int d = tid & (kDP - 1), g = tid >> 6;
            float part = 0.f;
            if (d < D)
                for (int r = g; r < N; r += kT / kDP) part += Zp[(long)r * D + d] * (Yp[r] - mu);
            spart[g * kDP + d] = part;
        }
        __syncthreads();
        if (tid < kDP) sp[tid] = (spart[tid] + spart[kDP + tid]) + (spart[2 * kDP + tid] + spart[3 * kDP + tid]);

        // ---- the jitter ladder: form A, factor; a bad pivot ends the attempt for the whole workgroup
        int bad = 0;
        float jit = 0.f, s = 0.f;
        for (int attempt = 0; attempt <= a.max_tries; ++attempt) {
            jit = dkt_jitter_rung(a.jitter0, attempt);
            s = nz + jit;
            const float lam = s / v;
            __syncthreads();                       // (sp; the reads of the attempt before)
            for (int idx = tid; idx < D * D; idx += kT) {
                const int i = idx / D, j = idx - i * D;
                if (j <= i) sA[i * kDPP + j] = Sg[i * kDP + j] + (i == j ? lam : 0.f);
            }
            if (tid < D) sA[D * kDPP + tid] = sp[tid];
            __syncthreads();
            bad = cholesky_lower_rows<kT, true>(sA, sd, D, D + 1, kDPP, tid);
            if (!bad && N > D && !(s > 0.f)) bad = D + 1;          // (K = sv Z Z^T + s I has the eigenvalue s when N > D)
            if (!bad) break;
        }
        if (tid == 0) {
            a.info[prob] = bad;
            a.jit[prob] = jit;
        }
        if (bad) {                                 // every rung failed: NaN (the dZ of the episode at the end)
            anybad = true;
            if (tid == 0) {
                a.loo[prob] = nan;
                if (grad) {
                    a.dsv[prob] = nan;
                    a.dmean[prob] = nan;
                    a.dnoise[prob] = nan;
                }
            }
            for (int i = tid; i < N; i += kT) {
                alp[i] = nan;
                mup[i] = nan;
                varp[i] = nan;
            }
            continue;
        }
        if (tid < kDP) {
            st[tid] = tid < D ? sA[D * kDPP + tid] : 0.f;
            if (tid < D) seed_upper_diagonal(sA, sd, tid, kDPP);
        }
        __syncthreads();
        // U = L^-T into the upper triangle, a row per thread and no barrier inside (dkt_lds_dense.h);  w = U t from the finished row
        upper_inverse_rows(sA, sd, D, kDPP, tid);
        if (tid < kDP) sw[tid] = tid < D ? upper_row_dot(sA, st, tid, D, kDPP) : 0.f;
        __syncthreads();
        // G = U U^T over the lower triangle, its diagonal in sr ... mirrored into a dense matrix, zero past D
        gram_of_upper<kT>(sA, sr, D, kDPP, tid);
        __syncthreads();
        for (int idx = tid; idx < kDP * kDP; idx += kT) {
            const int i = idx / kDP, j = idx - i * kDP;
            float g = 0.f;
            if (i < D && j < D) g = i == j ? sr[i] : (j < i ? sA[i * kDPP + j] : sA[j * kDPP + i]);
            sG[i * kLd + j] = g;
        }
        __syncthreads();

        // ---- pass 2: the leave-one-out predictions of every row, the sums over the rows, M
        float accM[4][4] = {};
        float gwacc = 0.f, t0 = 0.f, t1 = 0.f, t2 = 0.f;
        const float4 w4 = *reinterpret_cast<const float4*>(sw + 4 * tx);
        for (int i0 = 0; i0 < N; i0 += kR) {
            stage_rows(sZ, Zp, i0, N, D, tid);
            __syncthreads();
            const int rows = min(kR, N - i0);
            float acc[4][4] = {};
            tile_ab(acc, sZ, sG, D, ty, tx);
            float h[4], zw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 z = *reinterpret_cast<const float4*>(sZ + (4 * ty + i) * kLd + 4 * tx);
                h[i] = group_sum16((acc[i][0] * z.x + acc[i][1] * z.y) + (acc[i][2] * z.z + acc[i][3] * z.w));
                zw[i] = group_sum16((w4.x * z.x + w4.y * z.y) + (w4.z * z.z + w4.w * z.w));
            }
            if (tx == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rl = 4 * ty + i, row = i0 + rl;
                    float av = 0.f, cv = 0.f, e0 = 0.f, e2 = 0.f;
                    if (row < N) {
                        const float y = Yp[row];
                        const float al = ((y - mu) - zw[i]) / s;
                        const float var = s / (1.f - h[i]);
                        av = -al * var;
                        const float bq = 0.5f * (var + av * av);
                        cv = -bq / s;
                        alp[row] = al;
                        mup[row] = y + av;
                        varp[row] = var;
                        e0 = -0.5f * logf(var) - 0.5f * al * al * var;
                        e2 = av * al + bq / var;
                    }
                    sa_[rl] = av;
                    sc_[rl] = cv;
                    sterm[rl] = e0;
                    sterm[kDP + rl] = av;
                    sterm[2 * kDP + rl] = e2;
                }
            }
            __syncthreads();
            if (tid < kDP) {                       // (wave 0: lane l sums row l of every block, the blocks in index order)
                t0 += sterm[tid];
                t1 += sterm[kDP + tid];
                t2 += sterm[2 * kDP + tid];
                if (grad)
                    for (int r = 0; r < rows; ++r) gwacc += sa_[r] * sZ[r * kLd + tid];
            }
            if (grad) tile_atb<true>(accM, sZ, sZ, sc_, rows, ty, tx);
            __syncthreads();
        }
        t0 = wave_sum(t0);
        t1 = wave_sum(t1);
        t2 = wave_sum(t2);
        if (tid == 0) a.loo[prob] = t0 - (float)N * kHalfLog2Pi;
        if (!grad) continue;

        // ---- gw = -(Z^T a) / s, gp = G gw, Q = -G (M + 1/2 (gw p^T + p gw^T)) G
        if (tid < kDP) sgw[tid] = -gwacc / s;
        __syncthreads();
        if (tid < kDP) {
            float g = 0.f;
            for (int k = 0; k < D; ++k) g += sG[k * kLd + tid] * sgw[k];
            sgp[tid] = g;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gi = 4 * ty + i, gj = 4 * tx + j;
                sM[gi * kLd + gj] = accM[i][j] + 0.5f * (sgw[gi] * sp[gj] + sp[gi] * sgw[gj]);
            }
        __syncthreads();
        {
            float acc[4][4] = {};
            tile_atb<false>(acc, sM, sG, nullptr, D, ty, tx);          // M G (M is symmetric up to rounding: its transpose is read)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *reinterpret_cast<float4*>(sQ + (4 * ty + i) * kLd + 4 * tx) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        }
        __syncthreads();
        {
            float acc[4][4] = {};
            tile_atb<false>(acc, sQ, sG, nullptr, D, ty, tx);          // (M G)^T G = G M G
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<float4*>(sQ + (4 * ty + i) * kLd + 4 * tx) = make_float4(-acc[i][0], -acc[i][1], -acc[i][2], -acc[i][3]);
                if (ty == tx) sred[4 * ty + i] = -acc[i][i];
            }
        }
        __syncthreads();
        {
            const float trq = wave_sum(sred[lane]), zg = wave_sum(szs[lane] * sgp[lane]);
            if (tid == 0) {
                a.dsv[prob] = -trq * s / (v * v);
                a.dmean[prob] = -t1 / s - zg;
                a.dnoise[prob] = -t2 / s + trq / v;
            }
        }

        // ---- pass 3: dZ_blk (+)= cls_weight_c (2 c_i G z_i + 2 Q z_i - (a_i / s) w + r_i gp), the classes in index order
        const float4 gp4 = *reinterpret_cast<const float4*>(sgp + 4 * tx);
        const float wv[4] = {w4.x, w4.y, w4.z, w4.w}, gv[4] = {gp4.x, gp4.y, gp4.z, gp4.w};
        for (int i0 = 0; i0 < N; i0 += kR) {
            stage_rows(sZ, Zp, i0, N, D, tid);
            if (tid < kR) {
                const int row = i0 + tid;
                float x0 = 0.f, x1 = 0.f, x2 = 0.f;
                if (row < N) {
                    const float al = alp[row], var = varp[row];
                    const float av = -al * var;
                    const float bq = 0.5f * (var + av * av);
                    x0 = 2.f * (-bq / s);
                    x1 = -av / s;
                    x2 = Yp[row] - mu;
                }
                sx0[tid] = x0;
                sx1[tid] = x1;
                sx2[tid] = x2;
            }
            __syncthreads();
            float a1[4][4] = {}, a2[4][4] = {};
#pragma unroll 2
            for (int k = 0; k < D; ++k) {
                const float4 g4 = *reinterpret_cast<const float4*>(sG + k * kLd + 4 * tx);
                const float4 q4 = *reinterpret_cast<const float4*>(sQ + k * kLd + 4 * tx);
                const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, qq[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float z = sZ[(4 * ty + i) * kLd + k];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        a1[i][j] += z * gg[j];
                        a2[i][j] += z * qq[j];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = 4 * ty + i, row = i0 + rl;
                if (row < N && 4 * tx < D) {
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = wc * ((sx0[rl] * a1[i][j] + 2.f * a2[i][j]) + (sx1[rl] * wv[j] + sx2[rl] * gv[j]));
                    float4* dst = reinterpret_cast<float4*>(dZp + (long)row * D + 4 * tx);
                    if (c > 0) {
                        const float4 p = *dst;
                        *dst = make_float4(p.x + o[0], p.y + o[1], p.z + o[2], p.w + o[3]);
                    } else {
                        *dst = make_float4(o[0], o[1], o[2], o[3]);
                    }
                }
            }
            __syncthreads();
        }
    }
    if (grad && anybad)
        for (long idx = tid; idx < (long)N * D; idx += kT) dZp[idx] = nan;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool loofs_shape_ok(int C, int N, int D) { return N >= 1 && D >= 1 && D <= DKT_LOOFS_MAX_D && D % 4 == 0 && C >= 1 && C <= DKT_LOOFS_MAX_C; }

}  // namespace

extern "C" int dkt_loofs_abi_version(void) { return DKT_LOOFS_ABI_VERSION; }

extern "C" size_t dkt_loofs_workspace_bytes(int B, int C, int N, int D) {
    if (B <= 0 || !loofs_shape_ok(C, N, D)) return 0;
    return (size_t)B * kDP * kDP * sizeof(float);
}

extern "C" int dkt_loofs_f32(const float* Z, const float* Y, long y_bstride, const float* sv, const float* mean, const float* noise,
                             const float* cls_weight, int B, int C, int N, int D, float jitter0, int max_tries, unsigned flags, float* loo,
                             float* alpha, float* mu_loo, float* var_loo, float* dZ, float* dsv, float* dmean, float* dnoise, float* jitter_used,
                             int32_t* info, void* workspace, size_t workspace_bytes, void* stream) {
    if (!Z || !Y || !sv || !mean || !noise || !loo || !alpha || !mu_loo || !var_loo || !jitter_used || !info || B <= 0 || max_tries < 0)
        return DKT_ERR_BAD_ARG;
    if (flags & ~DKT_LOOFS_WANT_GRAD) return DKT_ERR_BAD_ARG;
    const bool grad = flags & DKT_LOOFS_WANT_GRAD;
    if (grad && (!dZ || !dsv || !dmean || !dnoise)) return DKT_ERR_BAD_ARG;
    if (!loofs_shape_ok(C, N, D)) return DKT_ERR_SHAPE;
    if (y_bstride < 0 || (y_bstride != 0 && y_bstride < (long)C * N)) return DKT_ERR_BAD_ARG;
    if (!aligned16(Z) || (grad && !aligned16(dZ))) return DKT_ERR_BAD_ARG;
    if (!workspace || !aligned16(workspace) || workspace_bytes < dkt_loofs_workspace_bytes(B, C, N, D)) return DKT_ERR_WORKSPACE;
    const size_t lds = loofs_lds_bytes();
    if (set_lds((const void*)loofs_kernel, lds) != DKT_OK) return DKT_ERR_LAUNCH;
    const LoofsArgs a = {Z, Y, sv, mean, noise, cls_weight, loo, alpha, mu_loo, var_loo, dZ, dsv, dmean, dnoise, jitter_used, (float*)workspace, info,
                         y_bstride, C, N, D, max_tries, jitter0, flags};
    hipLaunchKernelGGL(loofs_kernel, dim3((unsigned)B), dim3(kT), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}
