// dkt_augment.hip -- libdkt_data.so: the episode image transform of the image-dataset loader (include/dkt_abi_data.h).
//
// Bit-exact Pillow arithmetic (docs/DATA_PIPELINE.md):
//   resize   ImagingResample's bilinear path: per output index, center = (x + 0.5) * scale, support = max(scale, 1), taps [xmin, xmax) clamped to the source
//            window, triangle weights in double normalised by their sum, quantised to 22-bit fixed point; horizontal pass first into a uint8
//            intermediate, then the vertical pass, each output clamp((2^21 + sum px * k) >> 22, 0, 255) in int32.
//   enhance  ImagingBlend: t = (float)d + (float)a * ((float)p - (float)d), 0 if t <= 0, 255 if t >= 255, else truncated.
//            Brightness d = 0; Contrast d = int(mean(L) + 0.5) over the whole image after brightness; Color d = the pixel's L;
//            L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
//   tensor   (u8 / 255 - mean) / std, IEEE fp32 divisions (hipcc's default correctly rounded divide; no fast-math).
// Floating-point contraction is off wherever it could fuse a multiply into an add (the coefficients and the blends): Pillow's C is built without FMA.
//
// Launch 1, aug_coeff_kernel: one thread per (image, axis, output index of the S-window) writes that index's tap window and 22-bit weights to the
//   workspace.  Launch 2, aug_image_kernel: one workgroup per image.  It walks the S output rows in bands whose uint8 intermediate rows fit in LDS
//   (a single output row always does: its taps span at most 2 h / rh + 2 rows and S <= rh, so rows * S * 3 <= 3 (2 h + 2 S) < INTER_BYTES), runs the
//   horizontal pass for the band's rows into LDS, then the vertical pass (+ Brightness, + the Contrast sum) to the output; with jitter, a final sweep
//   applies Contrast and Color to the workgroup's own output and normalises.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/dkt_abi.h"
#include "../../include/dkt_abi_data.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kInterBytes = 104 * 1024;
constexpr int kPrec = 22;

// Pillow's ksize for one axis: 2 * ceil(support) + 1
__host__ __device__ inline int taps_for(int in, int out) {
    double scale = (double)in / (double)out;
    double support = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(support) * 2 + 1;
}

// workspace words of one image (4-aligned): xmin, xn, ymin, yn [S] each, kx [S][Kx], ky [S][Ky]
__host__ __device__ inline int64_t image_words(int S, int Kx, int Ky) {
    int64_t w = 4 * (int64_t)S + (int64_t)S * (Kx + Ky);
    return (w + 3) & ~(int64_t)3;
}

// the limits of include/dkt_abi_data.h, except ws_off
__host__ __device__ inline bool entry_ok(const int64_t* e, int S, uint64_t pool_bytes) {
    const int64_t off = e[0], H = e[1], W = e[2], y0 = e[3], x0 = e[4], h = e[5], w = e[6], rh = e[7], rw = e[8], oy = e[9], ox = e[10];
    if (H < 1 || W < 1 || H > DKT_AUG_MAX_SIDE || W > DKT_AUG_MAX_SIDE) return false;
    if (y0 < 0 || x0 < 0 || h < 1 || w < 1 || y0 + h > H || x0 + w > W) return false;
    if (rh < S || rw < S || rh > DKT_AUG_MAX_SIDE || rw > DKT_AUG_MAX_SIDE) return false;
    if (oy < 0 || ox < 0 || oy + S > rh || ox + S > rw) return false;
    if (off < 0 || (uint64_t)off > pool_bytes || (uint64_t)(H * W * 3) > pool_bytes - (uint64_t)off) return false;
    return true;
}

__device__ inline int clip8(int acc) {
    int v = acc >> kPrec;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ inline int blend(int d, int p, float a) {
#pragma clang fp contract(off)
    float t = (float)d + a * ((float)p - (float)d);
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ inline int gray(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ inline float to_normalized(int v, float m, float s) {
#pragma clang fp contract(off)
    float x = (float)v / 255.0f;
    return (x - m) / s;
}

// one output index of one axis: tap window + quantised triangle weights (ImagingResample precompute_coeffs + normalize_coeffs_8bpc)
__global__ void __launch_bounds__(256) aug_coeff_kernel(const int64_t* __restrict__ table, int B, int S, uint64_t pool_bytes,
                                                         int* __restrict__ ws, int64_t ws_words) {
#pragma clang fp contract(off)
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)B * 2 * S) return;
    const int b = (int)(gid / (2 * S)), rem = (int)(gid - (int64_t)b * 2 * S), axis = rem / S, t = rem - axis * S;
    const int64_t* e = table + (int64_t)b * DKT_AUG_COLS;
    if (!entry_ok(e, S, pool_bytes)) return;
    const int Kx = taps_for((int)e[6], (int)e[8]), Ky = taps_for((int)e[5], (int)e[7]);
    const int64_t base = e[11];
    if (base < 0 || (base & 3) || base + image_words(S, Kx, Ky) > ws_words) return;
    const int in = axis == 0 ? (int)e[6] : (int)e[5];
    const int outsz = axis == 0 ? (int)e[8] : (int)e[7];
    const int o = axis == 0 ? (int)e[10] : (int)e[9];
    const int K = axis == 0 ? Kx : Ky;
    int* lo = ws + base + (axis == 0 ? 0 : 2 * S);
    int* kk = ws + base + 4 * S + (axis == 0 ? 0 : (int64_t)S * Kx) + (int64_t)t * K;

    const double scale = (double)in / (double)outsz;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = filterscale;           // bilinear: support 1
    const int xx = o + t;
    const double center = 0.0 + (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        double u = (x + xmin - center + 0.5) * ss;
        if (u < 0.0) u = -u;
        ww += u < 1.0 ? 1.0 - u : 0.0;
    }
    for (int x = 0; x < K; ++x) {
        int q = 0;
        if (x < xmax) {
            double u = (x + xmin - center + 0.5) * ss;
            if (u < 0.0) u = -u;
            double w = u < 1.0 ? 1.0 - u : 0.0;
            if (ww != 0.0) w /= ww;
            q = w < 0.0 ? (int)(-0.5 + w * (1 << kPrec)) : (int)(0.5 + w * (1 << kPrec));
        }
        kk[x] = q;
    }
    lo[t] = xmin;
    lo[S + t] = xmax;
}

template <bool JIT>
__global__ void __launch_bounds__(kThreads) aug_image_kernel(const uint8_t* __restrict__ pool, uint64_t pool_bytes, const int64_t* __restrict__ table,
                                                             const float* __restrict__ jitter, const uint8_t* __restrict__ flip, int S,
                                                             float m0, float m1, float m2, float s0, float s1, float s2,
                                                             float* __restrict__ out, const int* __restrict__ ws, int64_t ws_words) {
    __shared__ uint8_t inter[kInterBytes];
    __shared__ int red[kThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t SS = (int64_t)S * S;
    float* ob = out + (int64_t)b * 3 * SS;
    const int64_t* e = table + (int64_t)b * DKT_AUG_COLS;
    bool ok = entry_ok(e, S, pool_bytes);
    int Kx = 0, Ky = 0;
    if (ok) {
        Kx = taps_for((int)e[6], (int)e[8]);
        Ky = taps_for((int)e[5], (int)e[7]);
        ok = e[11] >= 0 && !(e[11] & 3) && e[11] + image_words(S, Kx, Ky) <= ws_words;
    }
    if (!ok) {                                     // an entry the host did not plan: NaN, and no access outside the pool
        for (int64_t i = tid; i < 3 * SS; i += kThreads) ob[i] = __builtin_nanf("");
        return;
    }
    const uint8_t* img = pool + e[0];
    const int W = (int)e[2], y0 = (int)e[3], x0 = (int)e[4];
    const int* xmin = ws + e[11];
    const int* xn = xmin + S;
    const int* ymin = xmin + 2 * S;
    const int* yn = xmin + 3 * S;
    const int* kx = xmin + 4 * S;
    const int* ky = kx + (int64_t)S * Kx;
    float ab = 1.0f, ac = 1.0f, as = 1.0f;
    if (JIT) {
        ab = jitter[3 * b + 0];
        ac = jitter[3 * b + 1];
        as = jitter[3 * b + 2];
    }
    const bool fl = flip != nullptr && flip[b] != 0;
    const int cap_rows = kInterBytes / (S * 3);
    int lsum = 0;

    for (int y0p = 0; y0p < S;) {
        const int r0 = ymin[y0p];
        int y1p = y0p + 1;
        while (y1p < S && ymin[y1p] + yn[y1p] - r0 <= cap_rows) ++y1p;
        const int rows = ymin[y1p - 1] + yn[y1p - 1] - r0;
        if (rows > cap_rows) break;                // cannot happen within the limits (see the file comment)
        __syncthreads();                           // the previous band's vertical pass has read `inter`
        for (int it = tid; it < rows * S; it += kThreads) {
            const int r = it / S, t = it - r * S;
            const int n = xn[t];
            const int* k = kx + (int64_t)t * Kx;
            const uint8_t* p = img + ((int64_t)(y0 + r0 + r) * W + x0 + xmin[t]) * 3;
            int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
            for (int i = 0; i < n; ++i) {
                const int w = k[i];
                a0 += (int)p[3 * i + 0] * w;
                a1 += (int)p[3 * i + 1] * w;
                a2 += (int)p[3 * i + 2] * w;
            }
            uint8_t* q = inter + (r * S + t) * 3;
            q[0] = (uint8_t)clip8(a0);
            q[1] = (uint8_t)clip8(a1);
            q[2] = (uint8_t)clip8(a2);
        }
        __syncthreads();
        for (int it = tid; it < (y1p - y0p) * S; it += kThreads) {
            const int yr = it / S, t = it - yr * S, yo = y0p + yr;
            const int n = yn[yo];
            const int* k = ky + (int64_t)yo * Ky;
            const uint8_t* q = inter + ((ymin[yo] - r0) * S + t) * 3;
            int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
            for (int j = 0; j < n; ++j) {
                const int w = k[j];
                a0 += (int)q[j * S * 3 + 0] * w;
                a1 += (int)q[j * S * 3 + 1] * w;
                a2 += (int)q[j * S * 3 + 2] * w;
            }
            int v0 = clip8(a0), v1 = clip8(a1), v2 = clip8(a2);
            const int64_t o = (int64_t)yo * S + (fl ? S - 1 - t : t);
            if (JIT) {
                v0 = blend(0, v0, ab);
                v1 = blend(0, v1, ab);
                v2 = blend(0, v2, ab);
                lsum += gray(v0, v1, v2);
                ob[o] = (float)v0;                 // parked until the Contrast mean is known; re-read by this workgroup after the barriers below
                ob[SS + o] = (float)v1;
                ob[2 * SS + o] = (float)v2;
            } else {
                ob[o] = to_normalized(v0, m0, s0);
                ob[SS + o] = to_normalized(v1, m1, s1);
                ob[2 * SS + o] = to_normalized(v2, m2, s2);
            }
        }
        y0p = y1p;
    }
    if (!JIT) return;

    // exact integer sum of L over the image (S * S * 255 < 2^31)
    for (int d = 32; d > 0; d >>= 1) lsum += __shfl_down(lsum, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = lsum;
    __syncthreads();
    int total = 0;
    for (int w = 0; w < kThreads / 64; ++w) total += red[w];
    const int mean = (int)((double)total / (double)SS + 0.5);
    for (int64_t i = tid; i < SS; i += kThreads) {
        int c0 = blend(mean, (int)ob[i], ac);
        int c1 = blend(mean, (int)ob[SS + i], ac);
        int c2 = blend(mean, (int)ob[2 * SS + i], ac);
        const int l = gray(c0, c1, c2);
        ob[i] = to_normalized(blend(l, c0, as), m0, s0);
        ob[SS + i] = to_normalized(blend(l, c1, as), m1, s1);
        ob[2 * SS + i] = to_normalized(blend(l, c2, as), m2, s2);
    }
}

// validates every entry, recomputes the workspace layout; `check_off` compares it with the table's ws_off column, otherwise writes it there
int plan_table(int64_t* tw, const int64_t* tr, int B, int S, uint64_t pool_bytes, bool check_off, int64_t* words) {
    int64_t acc = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t* e = tr + (int64_t)b * DKT_AUG_COLS;
        if (!entry_ok(e, S, pool_bytes)) return DKT_ERR_BAD_ARG;
        const int64_t n = image_words(S, taps_for((int)e[6], (int)e[8]), taps_for((int)e[5], (int)e[7]));
        if (check_off) {
            if (e[11] != acc) return DKT_ERR_BAD_ARG;
        } else {
            tw[(int64_t)b * DKT_AUG_COLS + 11] = acc;
        }
        acc += n;
    }
    *words = acc;
    return DKT_OK;
}

bool finite_nonzero(float v) { return std::isfinite(v) && v != 0.0f; }

}  // namespace

extern "C" int dkt_data_abi_version(void) { return DKT_DATA_ABI_VERSION; }

extern "C" int dkt_augment_plan(int64_t* table, int B, int S, size_t* ws_bytes) {
    if (!table || !ws_bytes || B < 1 || S < 1 || S > DKT_AUG_MAX_S) return DKT_ERR_BAD_ARG;
    if (B > (1 << 20)) return DKT_ERR_TOO_LARGE;
    int64_t words = 0;
    int st = plan_table(table, table, B, S, UINT64_MAX, false, &words);
    if (st != DKT_OK) return st;
    *ws_bytes = (size_t)words * 4;
    return DKT_OK;
}

extern "C" int dkt_augment_u8(const uint8_t* pool, size_t pool_bytes, const int64_t* table_host, const int64_t* table_dev, int B, const float* jitter,
                              const uint8_t* flip, int S, const float* mean, const float* std, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!pool || !pool_bytes || !table_host || !table_dev || !mean || !std || !out || !ws) return DKT_ERR_BAD_ARG;
    if (B < 1 || S < 1 || S > DKT_AUG_MAX_S) return DKT_ERR_BAD_ARG;
    if (B > (1 << 20)) return DKT_ERR_TOO_LARGE;
    if (((uintptr_t)out & 3) || ((uintptr_t)ws & 15) || (jitter && ((uintptr_t)jitter & 3)) || ((uintptr_t)table_dev & 7)) return DKT_ERR_BAD_ARG;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(mean[c]) || !finite_nonzero(std[c])) return DKT_ERR_BAD_ARG;
    int64_t words = 0;
    int st = plan_table(nullptr, table_host, B, S, pool_bytes, true, &words);
    if (st != DKT_OK) return st;
    if ((uint64_t)words * 4 > ws_bytes) return DKT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nthreads = (int64_t)B * 2 * S;
    hipLaunchKernelGGL(aug_coeff_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, table_dev, B, S, (uint64_t)pool_bytes, (int*)ws,
                       (int64_t)(ws_bytes / 4));
    if (hipGetLastError() != hipSuccess) return DKT_ERR_LAUNCH;
    if (jitter)
        hipLaunchKernelGGL(aug_image_kernel<true>, dim3(B), dim3(kThreads), 0, s, pool, (uint64_t)pool_bytes, table_dev, jitter, flip, S,
                           mean[0], mean[1], mean[2], std[0], std[1], std[2], out, (const int*)ws, (int64_t)(ws_bytes / 4));
    else
        hipLaunchKernelGGL(aug_image_kernel<false>, dim3(B), dim3(kThreads), 0, s, pool, (uint64_t)pool_bytes, table_dev, jitter, flip, S,
                           mean[0], mean[1], mean[2], std[0], std[1], std[2], out, (const int*)ws, (int64_t)(ws_bytes / 4));
    return hipGetLastError() == hipSuccess ? DKT_OK : DKT_ERR_LAUNCH;
}
