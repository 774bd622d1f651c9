// One 16-byte channel group per lane access, shared by the streaming NHWC kernels (nn, conv3d, packnet, bts, google, motion, dense;
// conv.hip takes VecOf only).  Device side only; the host side of a streaming file is launch.h.
#pragma once
#include "common.h"

// elements of T in 16 bytes
template <typename T> struct VecOf;
template <> struct VecOf<float> { static constexpr int V = 4; };
template <> struct VecOf<bf16_t> { static constexpr int V = 8; };
template <> struct VecOf<half_t> { static constexpr int V = 8; };

// 16 bytes of ES-byte elements, as raw bits (for kernels that only move / zero / add elements)
template <int ES> struct Bits;
template <> struct Bits<2> { typedef unsigned short E; static constexpr int V = 8; };
template <> struct Bits<4> { typedef unsigned int E; static constexpr int V = 4; };

// 16 bytes at p <-> VecOf<T>::V floats
template <typename T> __device__ __forceinline__ void load_vec(const T* p, float* v);
template <> __device__ __forceinline__ void load_vec<float>(const float* p, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <> __device__ __forceinline__ void load_vec<bf16_t>(const bf16_t* p, float* v) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(w[i] << 16);
        v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}
template <> __device__ __forceinline__ void load_vec<half_t>(const half_t* p, float* v) {
    typedef __attribute__((ext_vector_type(8))) _Float16 h8;
    const h8 t = *reinterpret_cast<const h8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
}
// The same in two steps, for kernels that keep several loads in flight: load_raw16 only issues the load (4 registers, nothing waits), unpack_vec converts
// at the point of use.  unpack_vec<T>(load_raw16(p), v) gives the floats of load_vec<T>(p, v).
template <typename T> __device__ __forceinline__ uint4 load_raw16(const T* p) { return *reinterpret_cast<const uint4*>(p); }
template <typename T> __device__ __forceinline__ void unpack_vec(const uint4& t, float* v);
template <> __device__ __forceinline__ void unpack_vec<bf16_t>(const uint4& t, float* v) {
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(w[i] << 16);
        v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}
template <> __device__ __forceinline__ void unpack_vec<half_t>(const uint4& t, float* v) {
    typedef __attribute__((ext_vector_type(8))) _Float16 h8;
    const h8 h = __builtin_bit_cast(h8, t);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
}
template <typename T> __device__ __forceinline__ void store_vec(T* p, const float* v);
template <> __device__ __forceinline__ void store_vec<float>(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void store_vec<bf16_t>(bf16_t* p, const float* v) {
    bf16_t o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (bf16_t)v[i];
    *reinterpret_cast<uint4*>(p) = *reinterpret_cast<uint4*>(o);
}
template <> __device__ __forceinline__ void store_vec<half_t>(half_t* p, const float* v) {
    typedef __attribute__((ext_vector_type(8))) _Float16 h8;
    h8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (_Float16)v[i];
    *reinterpret_cast<h8*>(p) = o;
}
