// dkt_frontend_big_kernels.h -- the streaming front-end kernels of episodes with more than 128 rows (dkt_frontend_big.hip), templated on the element type
// XT of the trunk output X and its gradient dX: XT = float in the product, __bf16 / _Float16 in libdkt_x16.so (dkt_frontend_x16.hip).  Only the loads
// of X and the stores of dX depend on XT (dkt_xio.h); Zn, dZn, the statistics and all arithmetic stay fp32.
#pragma once
#include "dkt_common.h"
#include "dkt_xio.h"
#include "../../include/dkt_abi.h"

namespace {

// one wave per row; up to D = 2048 the row's y = a x + s stays in the wave's registers between the norm and the store (X is read once), beyond that the row is
// read a second time (an L1 / L2 hit)
template <typename XT>
__global__ __launch_bounds__(256) void affine_normalize_kernel(const XT* __restrict__ X, const float* __restrict__ A, const float* __restrict__ S, long ab_bstride,
                                                               float* __restrict__ Zn, float* __restrict__ rnorm, long rows, int N, int D) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const long b = row / N;
    const XT* x = X + row * D;
    const float4* a = reinterpret_cast<const float4*>(A + b * ab_bstride);
    const float4* s = reinterpret_cast<const float4*>(S + b * ab_bstride);
    float4* z = reinterpret_cast<float4*>(Zn + row * D);
    const int nv = D >> 2;
    float ss = 0.f;
    if (nv <= 512) {
        float4 y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int v = lane + 64 * k;
            y[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (v < nv) {
                const float4 xv = xload4(x, v), av = a[v], sv = s[v];
                y[k] = make_float4(__builtin_fmaf(av.x, xv.x, sv.x), __builtin_fmaf(av.y, xv.y, sv.y), __builtin_fmaf(av.z, xv.z, sv.z), __builtin_fmaf(av.w, xv.w, sv.w));
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {      // (same order of the squares as the streaming form below: lane-wise v = lane, lane + 64, ...)
            ss = __builtin_fmaf(y[k].x, y[k].x, ss); ss = __builtin_fmaf(y[k].y, y[k].y, ss); ss = __builtin_fmaf(y[k].z, y[k].z, ss); ss = __builtin_fmaf(y[k].w, y[k].w, ss);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, DKT_WAVE);
        const float rn = 1.0f / fmaxf(sqrtf(ss), 1e-12f);        // F.normalize: x / max(|x|_2, eps)
        if (lane == 0) rnorm[row] = rn;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int v = lane + 64 * k;
            if (v < nv) z[v] = make_float4(y[k].x * rn, y[k].y * rn, y[k].z * rn, y[k].w * rn);
        }
        return;
    }
    for (int v = lane; v < nv; v += 64) {
        const float4 xv = xload4(x, v), av = a[v], sv = s[v];
        const float y0 = __builtin_fmaf(av.x, xv.x, sv.x), y1 = __builtin_fmaf(av.y, xv.y, sv.y), y2 = __builtin_fmaf(av.z, xv.z, sv.z), y3 = __builtin_fmaf(av.w, xv.w, sv.w);
        ss = __builtin_fmaf(y0, y0, ss); ss = __builtin_fmaf(y1, y1, ss); ss = __builtin_fmaf(y2, y2, ss); ss = __builtin_fmaf(y3, y3, ss);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, DKT_WAVE);
    const float rn = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    if (lane == 0) rnorm[row] = rn;
    for (int v = lane; v < nv; v += 64) {                     // (the second read of the row is an L1 / L2 hit)
        const float4 xv = xload4(x, v), av = a[v], sv = s[v];
        z[v] = make_float4(__builtin_fmaf(av.x, xv.x, sv.x) * rn, __builtin_fmaf(av.y, xv.y, sv.y) * rn, __builtin_fmaf(av.z, xv.z, sv.z) * rn,
                           __builtin_fmaf(av.w, xv.w, sv.w) * rn);
    }
}

// t[row] = Zn[row] . dZn[row]; one wave per row
__global__ __launch_bounds__(256) void rowdot_kernel(const float* __restrict__ Zn, const float* __restrict__ dZn, float* __restrict__ t, long rows, int D) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float4* z = reinterpret_cast<const float4*>(Zn + row * D);
    const float4* g = reinterpret_cast<const float4*>(dZn + row * D);
    float acc = 0.f;
    for (int v = lane; v < (D >> 2); v += 64) {
        const float4 zv = z[v], gv = g[v];
        acc = __builtin_fmaf(zv.x, gv.x, acc); acc = __builtin_fmaf(zv.y, gv.y, acc); acc = __builtin_fmaf(zv.z, gv.z, acc); acc = __builtin_fmaf(zv.w, gv.w, acc);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, DKT_WAVE);
    if (lane == 0) t[row] = acc;
}

// workgroup = (episode b, 32-feature slab): thread (r = tid >> 3, c4 = tid & 7) walks the rows r, r + 32, ... of its 4 features.
// TRAIN: first pass dY -> LDS + column sums, second pass dX from LDS (x re-read: an L2 hit); otherwise (eval-mode statistics / no bn_out) dX = a dY at once.
template <typename XT, bool TRAIN>
__global__ __launch_bounds__(256) void normalize_bn_bwd_cols_kernel(const float* __restrict__ dZn, const float* __restrict__ Zn, const XT* __restrict__ X,
                                                                    const float* __restrict__ A, long a_bstride, const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd, const float* __restrict__ rnorm, const float* __restrict__ t,
                                                                    XT* __restrict__ dX, float* __restrict__ dgamma_part, float* __restrict__ dbeta_part,
                                                                    int N, int D, int nslab) {
    extern __shared__ __attribute__((aligned(16))) float dy_s[];            // TRAIN: [N][32] | red[2][32][8 x 4]
    const int b = blockIdx.x / nslab, sl = blockIdx.x % nslab;
    const int tid = threadIdx.x, r = tid >> 3, c4 = tid & 7;
    const int d = 32 * sl + 4 * c4;
    const bool dok = d < D;                                                 // (D % 4 == 0: a float4 is inside the row or wholly beyond it)
    const size_t base = (size_t)b * N * D + d;
    const float4 av = dok ? *reinterpret_cast<const float4*>(A + (size_t)b * a_bstride + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), rs = mu;
    if (TRAIN && dok) {
        mu = *reinterpret_cast<const float4*>(mean + (size_t)b * D + d);
        rs = *reinterpret_cast<const float4*>(rstd + (size_t)b * D + d);
    }
    float4 sb = make_float4(0.f, 0.f, 0.f, 0.f), sg = sb;                   // column sums of dY and dY xhat over this thread's rows
    // four rows per trip, every load of the trip issued before the first use (round 6: one row per trip left each of the 16 waves of a CU waiting for its own
    // three loads, trip after trip -- 0.40 of the HBM roofline at the 20-way shape); rows past N are clamped to the last row and weighted out
    for (int i0 = r; i0 < N; i0 += 128) {
        float4 g[4], z[4], x[4];
        float ti[4], rn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = min(i0 + 32 * u, N - 1);
            const size_t o = base + (size_t)i * D;
            g[u] = z[u] = x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (dok) {
                g[u] = *reinterpret_cast<const float4*>(dZn + o);
                z[u] = *reinterpret_cast<const float4*>(Zn + o);
                if (TRAIN) x[u] = xload4(X + o);
            }
            ti[u] = t[(size_t)b * N + i];
            rn[u] = rnorm[(size_t)b * N + i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 32 * u;
            if (i < N) {
                float4 dy = make_float4(0.f, 0.f, 0.f, 0.f);
                if (dok) {
                    dy = make_float4(rn[u] * __builtin_fmaf(-z[u].x, ti[u], g[u].x), rn[u] * __builtin_fmaf(-z[u].y, ti[u], g[u].y),
                                     rn[u] * __builtin_fmaf(-z[u].z, ti[u], g[u].z), rn[u] * __builtin_fmaf(-z[u].w, ti[u], g[u].w));
                    if (TRAIN) {
                        sb.x += dy.x; sb.y += dy.y; sb.z += dy.z; sb.w += dy.w;
                        sg.x = __builtin_fmaf(dy.x, (x[u].x - mu.x) * rs.x, sg.x); sg.y = __builtin_fmaf(dy.y, (x[u].y - mu.y) * rs.y, sg.y);
                        sg.z = __builtin_fmaf(dy.z, (x[u].z - mu.z) * rs.z, sg.z); sg.w = __builtin_fmaf(dy.w, (x[u].w - mu.w) * rs.w, sg.w);
                    } else {
                        const float4 o = make_float4(av.x * dy.x, av.y * dy.y, av.z * dy.z, av.w * dy.w);
                        xstore4(dX + base + (size_t)i * D, o);
                    }
                }
                if (TRAIN) *reinterpret_cast<float4*>(dy_s + (size_t)i * 32 + 4 * c4) = dy;
            }
        }
    }
    if (!TRAIN) return;
    // the 32 row-threads of a feature quad: fixed-order tree over r in LDS (deterministic)
    float* red = dy_s + (size_t)N * 32;                                     // [32 rows r][8 c4][8]
    *reinterpret_cast<float4*>(red + (r * 8 + c4) * 8) = sb;
    *reinterpret_cast<float4*>(red + (r * 8 + c4) * 8 + 4) = sg;
    __syncthreads();
    for (int step = 16; step >= 1; step >>= 1) {
        if (r < step) {
            float* p = red + (r * 8 + c4) * 8;
            const float* qv = red + ((r + step) * 8 + c4) * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) p[e] += qv[e];
        }
        __syncthreads();
    }
    const float4 tb = *reinterpret_cast<const float4*>(red + c4 * 8), tg = *reinterpret_cast<const float4*>(red + c4 * 8 + 4);
    if (r == 0 && dok) {
        *reinterpret_cast<float4*>(dbeta_part + (size_t)b * D + d) = tb;
        *reinterpret_cast<float4*>(dgamma_part + (size_t)b * D + d) = tg;
    }
    if (!dok) return;
    const float inv_n = 1.0f / (float)N;
    for (int i0 = r; i0 < N; i0 += 128) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = xload4(X + base + (size_t)min(i0 + 32 * u, N - 1) * D);     // (second read of the slab: an L2 / MALL hit)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 32 * u;
            if (i < N) {
                const float4 dy = *reinterpret_cast<const float4*>(dy_s + (size_t)i * 32 + 4 * c4);
                float4 out;
                out.x = av.x * (dy.x - inv_n * (tb.x + (x[u].x - mu.x) * rs.x * tg.x));
                out.y = av.y * (dy.y - inv_n * (tb.y + (x[u].y - mu.y) * rs.y * tg.y));
                out.z = av.z * (dy.z - inv_n * (tb.z + (x[u].z - mu.z) * rs.z * tg.z));
                out.w = av.w * (dy.w - inv_n * (tb.w + (x[u].w - mu.w) * rs.w * tg.w));
                xstore4(dX + base + (size_t)i * D, out);
            }
        }
    }
}

// the launches behind dkt_affine_normalize_* / dkt_normalize_bn_bwd_* (the host checks are the callers')
template <typename XT>
int affine_normalize_launch(const XT* X, const float* a, const float* s, long ab_bstride, float* Zn, float* rnorm, long rows, int N, int D, hipStream_t st) {
    hipLaunchKernelGGL(affine_normalize_kernel<XT>, dim3((unsigned)((rows + 3) / 4)), dim3(256), dkt_lds_pad(DKT_SW_PAD_AFFNORM), st, X, a, s, ab_bstride, Zn, rnorm, rows, N, D);
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}

template <typename XT>
int normalize_bn_bwd_launch(const float* dZn, const float* Zn, const XT* X, const float* a, long a_bstride, const float* mean, const float* rstd, const float* rnorm,
                            XT* dX, float* dgamma_part, float* dbeta_part, float* rowdot_ws, int B, int N, int D, bool train, hipStream_t st) {
    const long rows = (long)B * N;
    const int nslab = (D + 31) / 32;
    hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), dkt_lds_pad(DKT_SW_PAD_ROWDOT), st, Zn, dZn, rowdot_ws, rows, D);
    if (train) {
        const size_t lds = ((size_t)N * 32 + 32 * 8 * 8) * sizeof(float);
        if (lds > 48 * 1024 &&
            hipFuncSetAttribute((const void*)normalize_bn_bwd_cols_kernel<XT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((1024 * 32 + 32 * 8 * 8) * sizeof(float))) != hipSuccess)
            return DKT_ERR_LAUNCH;
        hipLaunchKernelGGL((normalize_bn_bwd_cols_kernel<XT, true>), dim3((unsigned)(B * nslab)), dim3(256), lds, st, dZn, Zn, X, a, a_bstride, mean, rstd, rnorm, rowdot_ws, dX,
                           dgamma_part, dbeta_part, N, D, nslab);
    } else {
        hipLaunchKernelGGL((normalize_bn_bwd_cols_kernel<XT, false>), dim3((unsigned)(B * nslab)), dim3(256), dkt_lds_pad(DKT_SW_PAD_NBB), st, dZn, Zn, X, a, a_bstride, mean, rstd, rnorm, rowdot_ws, dX,
                           dgamma_part, dbeta_part, N, D, nslab);
    }
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}

}  // namespace
