// dkt_xio.h -- loads of the trunk output X and stores of its gradient dX in the element type XT of the front-end kernels (dkt_frontend_kernels.h,
// dkt_frontend_big_kernels.h): XT = float is the product's form (16-byte loads / stores, exactly the code those kernels had before they were
// templated); XT = __bf16 / _Float16 move 4 elements in 8 bytes.  Loads widen to fp32 exactly; stores round to nearest-even, overflow to +-inf
// (what Tensor.to(dtype) does; gfx950: v_cvt_pk_bf16_f32, v_cvt_f16_f32).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace {

typedef __amdgpu_buffer_rsrc_t brsrc_t;
__device__ __forceinline__ brsrc_t mk_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 bload4(brsrc_t r, int voff, int soff) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}
constexpr int OOB = 0x7ffffff0;
__device__ __forceinline__ void fe_store4(brsrc_t r, int voff, float a0, float a1, float a2, float a3) {     // soffset = literal 0: see bstore4, dkt_mfma_tiles.h
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {__float_as_uint(a0), __float_as_uint(a1), __float_as_uint(a2), __float_as_uint(a3)};
    __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, 0, 0);
}

// bytes per element of X / dX (the kernels' byte offsets and descriptor sizes scale with it)
template <typename XT>
constexpr int xbytes() { return (int)sizeof(XT); }

// two packed 16-bit elements -> two floats (exact)
template <typename XT>
__device__ __forceinline__ float2 widen2(unsigned w) {
    if constexpr (std::is_same_v<XT, __bf16>) {
        return make_float2(__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u));
    } else {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 h = __builtin_bit_cast(h2, w);
        return make_float2((float)h.x, (float)h.y);
    }
}
// two floats -> two packed 16-bit elements, round to nearest-even
template <typename XT>
__device__ __forceinline__ unsigned narrow2(float a, float b) {
    typedef XT x2 __attribute__((ext_vector_type(2)));
    const x2 h = {(XT)a, (XT)b};
    return __builtin_bit_cast(unsigned, h);
}
template <typename XT>
__device__ __forceinline__ float4 widen4(unsigned lo, unsigned hi) {
    const float2 a = widen2<XT>(lo), b = widen2<XT>(hi);
    return make_float4(a.x, a.y, b.x, b.y);
}

// 4 consecutive elements through a buffer descriptor (byte offsets): 16 B for float, 8 B for a 16-bit type
template <typename XT>
__device__ __forceinline__ float4 xbload4(brsrc_t r, int voff, int soff) {
    if constexpr (std::is_same_v<XT, float>) {
        return bload4(r, voff, soff);
    } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
        return widen4<XT>(v[0], v[1]);
    }
}
template <typename XT>
__device__ __forceinline__ void xbstore4(brsrc_t r, int voff, float a0, float a1, float a2, float a3) {
    if constexpr (std::is_same_v<XT, float>) {
        fe_store4(r, voff, a0, a1, a2, a3);
    } else {
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 v = {narrow2<XT>(a0, a1), narrow2<XT>(a2, a3)};
        __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, 0, 0);
    }
}

// 4 consecutive elements through a plain pointer (16-byte aligned for float, 8-byte for a 16-bit type); v counts groups of 4 elements from p
template <typename XT>
__device__ __forceinline__ float4 xload4(const XT* p) {
    if constexpr (std::is_same_v<XT, float>) {
        return *reinterpret_cast<const float4*>(p);
    } else {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
        return widen4<XT>(w.x, w.y);
    }
}
template <typename XT>
__device__ __forceinline__ float4 xload4(const XT* p, long v) {
    if constexpr (std::is_same_v<XT, float>) {
        return reinterpret_cast<const float4*>(p)[v];
    } else {
        const uint2 w = reinterpret_cast<const uint2*>(p)[v];
        return widen4<XT>(w.x, w.y);
    }
}
template <typename XT>
__device__ __forceinline__ void xstore4(XT* p, float4 y) {
    if constexpr (std::is_same_v<XT, float>) {
        *reinterpret_cast<float4*>(p) = y;
    } else {
        *reinterpret_cast<uint2*>(p) = make_uint2(narrow2<XT>(y.x, y.y), narrow2<XT>(y.z, y.w));
    }
}

}  // namespace
