// Wide accesses at any byte address, shared by the streaming kernels that walk an image flat (present.hip, flow.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ND dwords to / from any byte address, in the widest pieces: dwordx4 first, then one dwordx3 / x2 / x1.  The types carry no alignment promise:
// the compiler still emits global_load / global_store_dwordx2..4 for them, which this target serves at any address.
template <int K> struct VecAny { typedef uint32_t T __attribute__((ext_vector_type(K), aligned(1))); };
template <> struct VecAny<1> { typedef uint32_t T __attribute__((aligned(1))); };
template <int ND> __device__ __forceinline__ void put_dwords(void* dst, const uint32_t* w) {
    uint8_t* d = static_cast<uint8_t*>(dst);
    if constexpr (ND >= 4) {
        typename VecAny<4>::T v = {w[0], w[1], w[2], w[3]};
        *reinterpret_cast<typename VecAny<4>::T*>(d) = v;
        put_dwords<ND - 4>(d + 16, w + 4);
    } else if constexpr (ND == 3) {
        typename VecAny<3>::T v = {w[0], w[1], w[2]};
        *reinterpret_cast<typename VecAny<3>::T*>(d) = v;
    } else if constexpr (ND == 2) {
        typename VecAny<2>::T v = {w[0], w[1]};
        *reinterpret_cast<typename VecAny<2>::T*>(d) = v;
    } else if constexpr (ND == 1) {
        *reinterpret_cast<typename VecAny<1>::T*>(d) = w[0];
    }
}
template <int ND> __device__ __forceinline__ void get_dwords(const void* src, uint32_t* w) {
    const uint8_t* s = static_cast<const uint8_t*>(src);
    if constexpr (ND >= 4) {
        const typename VecAny<4>::T v = *reinterpret_cast<const typename VecAny<4>::T*>(s);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        get_dwords<ND - 4>(s + 16, w + 4);
    } else if constexpr (ND == 3) {
        const typename VecAny<3>::T v = *reinterpret_cast<const typename VecAny<3>::T*>(s);
        w[0] = v.x; w[1] = v.y; w[2] = v.z;
    } else if constexpr (ND == 2) {
        const typename VecAny<2>::T v = *reinterpret_cast<const typename VecAny<2>::T*>(s);
        w[0] = v.x; w[1] = v.y;
    } else if constexpr (ND == 1) {
        w[0] = *reinterpret_cast<const typename VecAny<1>::T*>(s);
    }
}
