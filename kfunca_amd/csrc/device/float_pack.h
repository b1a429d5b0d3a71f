// float <-> storage conversions shared by the row kernels (norm, cross-entropy, rope, gated activations, AdamW, index_add and the
// generic non-causal attention): 16-byte packs, per-element loads and stores, and the host's choice of the element type.
//
// The two bf16 stores differ in ONE thing, the bits of a NaN (both round to nearest even):
//   store_canonical   f32_to_bf16 (software): every NaN becomes 0x7FC0
//   store_hw          v_cvt_pk_bf16_f32 (one instruction, low half kept): a NaN keeps its sign and the top of its payload
// pack16 ALWAYS uses the hardware converter, so a kernel that stores packs with pack16 and single elements with store_canonical
// (norm, cross-entropy) writes different NaN bits on its two paths; rope, AdamW and the gated activations use store_hw and agree.
// For float and f16_t the two stores are the same.
#pragma once

#include "common.h"

namespace kf {

// elements of T in a 16-byte pack
template <typename T> constexpr int kPack16 = 16 / (int)sizeof(T);

template <typename T, int V>
__device__ __forceinline__ void unpack16(const uint4 &p, float (&f)[V]) {
    static_assert(V == kPack16<T>, "a pack is 16 bytes");
    if constexpr (sizeof(T) == 4) {
        f[0] = __uint_as_float(p.x); f[1] = __uint_as_float(p.y); f[2] = __uint_as_float(p.z); f[3] = __uint_as_float(p.w);
    } else {
        const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (std::is_same<T, bf16_t>::value) {
                f[2 * i] = __uint_as_float(w[i] << 16);
                f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
            } else {
                f[2 * i] = f16_to_f32(f16_t{(uint16_t)(w[i] & 0xffff)});
                f[2 * i + 1] = f16_to_f32(f16_t{(uint16_t)(w[i] >> 16)});
            }
        }
    }
}
template <typename T, int V>
__device__ __forceinline__ uint4 pack16(const float (&f)[V]) {
    static_assert(V == kPack16<T>, "a pack is 16 bytes");
    uint4 p;
    if constexpr (sizeof(T) == 4) {
        p.x = __float_as_uint(f[0]); p.y = __float_as_uint(f[1]); p.z = __float_as_uint(f[2]); p.w = __float_as_uint(f[3]);
    } else {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (std::is_same<T, bf16_t>::value) {
                w[i] = f32x2_to_bf16x2_hw(f[2 * i], f[2 * i + 1]);
            } else {
                const uint32_t lo = f32_to_f16(f[2 * i]).x, hi = f32_to_f16(f[2 * i + 1]).x;
                w[i] = lo | (hi << 16);
            }
        }
        p.x = w[0]; p.y = w[1]; p.z = w[2]; p.w = w[3];
    }
    return p;
}

template <typename T> __device__ __forceinline__ float load_f32(const T *p) { return (float)*p; }
template <> __device__ __forceinline__ float load_f32<bf16_t>(const bf16_t *p) { return bf16_to_f32(*p); }
template <> __device__ __forceinline__ float load_f32<f16_t>(const f16_t *p) { return f16_to_f32(*p); }

template <typename T> __device__ __forceinline__ void store_canonical(T *p, float v) { *p = (T)v; }
template <> __device__ __forceinline__ void store_canonical<bf16_t>(bf16_t *p, float v) { *p = f32_to_bf16(v); }
template <> __device__ __forceinline__ void store_canonical<f16_t>(f16_t *p, float v) { *p = f32_to_f16(v); }

template <typename T> __device__ __forceinline__ void store_hw(T *p, float v) { *p = (T)v; }
template <> __device__ __forceinline__ void store_hw<bf16_t>(bf16_t *p, float v) { p->x = (uint16_t)f32x2_to_bf16x2_hw(v, 0.f); }
template <> __device__ __forceinline__ void store_hw<f16_t>(f16_t *p, float v) { *p = f32_to_f16(v); }

// host: f(float{}), f(bf16_t{}) or f(f16_t{}) for a dtype the caller has checked to be one of the three, so that a generic lambda
// can name kernel<decltype(t)>
template <typename F> static inline int with_dtype(int dtype, F &&f) {
    return dtype == KF_F32 ? f(float{}) : dtype == KF_BF16 ? f(bf16_t{}) : f(f16_t{});
}

} // namespace kf
