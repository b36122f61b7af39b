// libdkt_loo.so (include/dkt_abi_loo.h; docs/LOO.md): the leave-one-out predictive log likelihood of B x C exact-GP problems
// K = sv_c E + (noise_c + jitter) I, its N leave-one-out predictions and its gradients, in ONE launch.
//
// ONE kernel instance, 256 threads, plain fp32 on the VALU, the problem held in LDS and inverted in place by the factor-and-invert family of
// csrc/dkt_lds_dense.h (the explanation is there): one (N + 1) x (N|1) matrix (64 KiB + 4.5 KiB of vectors at N = 127: two workgroups per CU).  Rows 0 .. N-1 hold the lower triangle of K, row N holds y - mean: the right-looking
// Cholesky sweep turns it into t = L^-1 (y - mean).  A pivot that is not finite and positive ends the attempt for the whole workgroup, which then
// forms K again with the next rung of the jitter ladder (0, jitter0, 10 jitter0, ...): decided per matrix, inside the kernel.  Then the inverse inside
// the factor's own storage: U = L^-T row by row into the upper triangle, alpha = U t, A = K^-1 = U U^T over the lower triangle, mirrored into the
// upper one (U is done with), so that every later product reads A along its rows: column i of A is row i, and the lanes of a wave read
// neighbouring words of one row.  loo, mu_loo, var_loo come from alpha and diag A.  Gradient: r = A q, and A diag(p) A in 4 x 4 register tiles over
// the lower triangle, G written to both triangles from the one value (bitwise symmetric); dsv, dnoise are sums over the same tiles.
// A workgroup serves one (episode, class) -- or, when the gradient of a SHARED E is asked for, the C classes of an episode one after the other: the
// thread that owns an element of W[b] adds the classes to it in index order (its own earlier write: no atomics, no workspace, a fixed order).
// Every reduction has a fixed order that depends on nothing but N.
#include "../../include/dkt_abi_loo.h"
#include "dkt_lds_dense.h"

namespace {

using namespace dkt_lds;                 // the factor-and-invert family of dkt_lds_dense.h, kWave, padded, wave_sum, kHalfLog2Pi, set_lds
constexpr int kT = 256;
constexpr int kVec = 128;
constexpr int kVecs = 9;                 // sd .. sred below

inline size_t loo_lds_bytes(int N) { return ((size_t)(N + 1) * padded(N) + kVecs * kVec) * sizeof(float); }

struct LooArgs {
    const float *E, *Y, *sv, *mean, *noise, *cw;
    float *loo, *alpha, *mu, *var, *W, *dsv, *dmean, *dnoise, *jit;
    int32_t* info;
    long ebs, ecs, ybs;
    int C, N, per_block, max_tries;      // per_block: classes a workgroup walks (C for the gradient of a shared E, else 1)
    float jitter0;
    unsigned flags;
};

// the 4 x 4 tile t of the lower triangle (tiles in row-major order of the triangle): tile row ti, tile column tj <= ti
__device__ __forceinline__ void tile_of(int t, int& ti, int& tj) {
    ti = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}

__global__ __launch_bounds__(kT) void loo_kernel(LooArgs a) {
    extern __shared__ float lds[];
    const int N = a.N, NP = padded(N), NN = N * N;
    float* sA = lds;                     // K (lower) + y - mean (row N) -> L (strict lower) + t (row N) -> U = L^-T (upper, diagonal included) -> A = K^-1 (all of it)
    float* sd = sA + (N + 1) * NP;       // pivots of L
    float* st = sd + kVec;               // t = L^-1 (y - mean)
    float* sa = st + kVec;               // alpha
    float* sr = sa + kVec;               // d = diag A
    float* sp = sr + kVec;               // p
    float* sq = sp + kVec;               // q
    float* sv_ = sq + kVec;              // r = A q
    float* sterm = sv_ + kVec;           // the terms of loo
    float* sred = sterm + kVec;          // cross-wave partials
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const bool grad = a.flags & DKT_LOO_WANT_GRAD;
    const bool shared = a.ecs == 0;
    const int nt = (N + 3) >> 2, ntl = nt * (nt + 1) / 2;
    const float nan = __builtin_nanf("");

    for (int cc = 0; cc < a.per_block; ++cc) {
        const long prob = (long)blockIdx.x * a.per_block + cc;
        const int b = (int)(prob / a.C), c = (int)(prob % a.C);
        const float* Ep = a.E + (long)b * a.ebs + (long)c * a.ecs;
        const float* Yp = a.Y + (long)b * a.ybs + (long)c * N;
        const float sc = a.sv[c], mu = a.mean[c], nz = a.noise[c];
        const float wc = a.cw ? a.cw[c] : 1.f;
        float* Wp = grad ? a.W + (shared ? (long)b : prob) * NN : nullptr;
        const bool add = shared && c > 0;          // W[b] of a shared E: this thread's own sum over the classes before

        // ---- the jitter ladder: form K, factor; a bad pivot ends the attempt for the whole workgroup
        int bad = 0;
        float jit = 0.f;
        for (int attempt = 0; attempt <= a.max_tries; ++attempt) {
            jit = dkt_jitter_rung(a.jitter0, attempt);
            __syncthreads();                       // (the reads of the attempt, or of the class, before)
            const float dg = nz + jit;
            stage_lower_rhs<kT>(sA, Ep, sc, [=](int) { return dg; }, [=](int i) { return Yp[i] - mu; }, N, NP, tid);
            __syncthreads();
            bad = cholesky_lower_rows<kT, true>(sA, sd, N, N + 1, NP, tid);
            if (!bad) break;
        }
        if (tid == 0) {
            a.info[prob] = bad;
            a.jit[prob] = jit;
        }
        if (bad) {                                 // every rung failed: NaN, through the same owners as the values (the W of a shared E is this thread's own sum)
            if (tid == 0) {
                a.loo[prob] = nan;
                if (grad) {
                    a.dsv[prob] = nan;
                    a.dmean[prob] = nan;
                    a.dnoise[prob] = nan;
                }
            }
            if (tid < N) {
                a.alpha[prob * N + tid] = nan;
                a.mu[prob * N + tid] = nan;
                a.var[prob * N + tid] = nan;
            }
            if (grad)
                for (int t = tid; t < ntl; t += kT) {
                    int ti, tj;
                    tile_of(t, ti, tj);
                    for (int x = 0; x < 4; ++x)
                        for (int y = 0; y < 4; ++y) {
                            const int i = 4 * ti + x, j = 4 * tj + y;
                            if (i < N && j <= i) {
                                Wp[i * N + j] = nan;
                                Wp[j * N + i] = nan;
                            }
                        }
                }
            continue;
        }
        if (tid < N) {
            st[tid] = sA[N * NP + tid];
            seed_upper_diagonal(sA, sd, tid, NP);
        }
        __syncthreads();
        // U = L^-T into the upper triangle, a row per thread and no barrier inside (dkt_lds_dense.h);  alpha = U t from the finished row
        upper_inverse_rows(sA, sd, N, NP, tid);
        if (tid < N) {
            const float al = upper_row_dot(sA, st, tid, N, NP);
            sa[tid] = al;
            a.alpha[prob * N + tid] = al;
        }
        __syncthreads();
        // A = U U^T over the lower triangle, its diagonal in sr
        gram_of_upper<kT>(sA, sr, N, NP, tid);
        __syncthreads();
        // ... mirrored into the upper triangle, the diagonal in its place: all of A, symmetric bit for bit
        for (int idx = tid; idx < NN; idx += kT) {
            int i = idx / N, j = idx - i * N;
            if (j < i) sA[j * NP + i] = sA[i * NP + j];
            else if (j == i) sA[i * NP + i] = sr[i];
        }
        // the leave-one-out predictions
        if (tid < N) {
            const float d = sr[tid], al = sa[tid], q = al / d;
            a.mu[prob * N + tid] = Yp[tid] - q;
            a.var[prob * N + tid] = 1.f / d;
            sterm[tid] = 0.5f * logf(d) - 0.5f * al * q;
            sp[tid] = 0.5f / d + 0.5f * q * q;
            sq[tid] = q;
        }
        __syncthreads();
        {
            const float s = sum_le128(sterm, N, lane);
            if (tid == 0) a.loo[prob] = s - (float)N * kHalfLog2Pi;
        }
        if (!grad) continue;
        // r = A q (row i of A read as its column: the lanes read neighbouring words)
        if (tid < N) {
            float acc = 0.f;
            for (int k = 0; k < N; ++k) acc += sA[k * NP + tid] * sq[k];
            sv_[tid] = acc;
        }
        __syncthreads();
        {
            const float s = sum_le128(sv_, N, lane);
            if (tid == 0) a.dmean[prob] = s;
        }
        // G = -A diag(p) A + 1/2 (alpha r^T + r alpha^T) over the lower triangle in 4 x 4 tiles;  W = cls_weight_c sv_c G,  dsv = <G, E>,  dnoise = tr G
        const float os = wc * sc;
        float dot = 0.f, tr = 0.f;
        for (int t = tid; t < ntl; t += kT) {
            int ti, tj;
            tile_of(t, ti, tj);
            int ia[4], ja[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                ia[x] = min(4 * ti + x, N - 1);                        // (rows past N repeat row N - 1: read, never written)
                ja[x] = min(4 * tj + x, N - 1);
            }
            float acc[4][4] = {};
#pragma unroll 2
            for (int k = 0; k < N; ++k) {
                const float* row = sA + k * NP;
                const float pk = sp[k];
                float av[4], bv[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    av[x] = row[ia[x]] * pk;
                    bv[x] = row[ja[x]];
                }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) acc[x][y] += av[x] * bv[y];
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const int i = 4 * ti + x, j = 4 * tj + y;
                    if (i < N && j <= i) {
                        const float g = 0.5f * (sa[i] * sv_[j] + sv_[i] * sa[j]) - acc[x][y];
                        const float w = __fmul_rn(os, g);          // (never contracted into the sum below: a shared W is the in-order sum of the per-class call's)
                        if (j == i) {
                            tr += g;
                            dot += g * Ep[i * N + i];
                            Wp[i * N + i] = add ? Wp[i * N + i] + w : w;
                        } else {
                            dot += g * (Ep[i * N + j] + Ep[j * N + i]);
                            Wp[i * N + j] = add ? Wp[i * N + j] + w : w;
                            Wp[j * N + i] = add ? Wp[j * N + i] + w : w;
                        }
                    }
                }
        }
        dot = wave_sum(dot);
        tr = wave_sum(tr);
        if (lane == 0) {
            sred[wave] = dot;
            sred[4 + wave] = tr;
        }
        __syncthreads();
        if (tid == 0) {
            a.dsv[prob] = block_sum4(sred);
            a.dnoise[prob] = block_sum4(sred + 4);
        }
    }
}

}  // namespace

extern "C" int dkt_loo_abi_version(void) { return DKT_LOO_ABI_VERSION; }

extern "C" int dkt_loo_f32(const float* E, long e_bstride, long e_cstride, const float* Y, long y_bstride, const float* sv, const float* mean,
                           const float* noise, const float* cls_weight, int B, int C, int N, float jitter0, int max_tries, unsigned flags,
                           float* loo, float* alpha, float* mu_loo, float* var_loo, float* W, float* dsv, float* dmean, float* dnoise,
                           float* jitter_used, int32_t* info, void* stream) {
    if (!E || !Y || !sv || !mean || !noise || !loo || !alpha || !mu_loo || !var_loo || !jitter_used || !info || B <= 0 || max_tries < 0)
        return DKT_ERR_BAD_ARG;
    if (flags & ~DKT_LOO_WANT_GRAD) return DKT_ERR_BAD_ARG;
    const bool grad = flags & DKT_LOO_WANT_GRAD;
    if (grad && (!W || !dsv || !dmean || !dnoise)) return DKT_ERR_BAD_ARG;
    if (N < 1 || N > DKT_LOO_MAX_N || C < 1 || C > DKT_LOO_MAX_C) return DKT_ERR_SHAPE;
    if (e_bstride < 0 || y_bstride < 0 || (e_cstride != 0 && e_cstride != (long)N * N)) return DKT_ERR_BAD_ARG;
    if ((long long)B * C > 0x7fffffffLL) return DKT_ERR_TOO_LARGE;
    const size_t lds = loo_lds_bytes(N);
    if (set_lds((const void*)loo_kernel, lds) != DKT_OK) return DKT_ERR_LAUNCH;
    const int per_block = (grad && e_cstride == 0) ? C : 1;
    const LooArgs a = {E, Y, sv, mean, noise, cls_weight, loo, alpha, mu_loo, var_loo, W, dsv, dmean, dnoise, jitter_used, info,
                       e_bstride, e_cstride, y_bstride, C, N, per_block, max_tries, jitter0, flags};
    hipLaunchKernelGGL(loo_kernel, dim3((unsigned)((long long)B * C / per_block)), dim3(kT), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}
