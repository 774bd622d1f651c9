// Host side of a streaming kernel file: the 1-D grid, the elements per 16-byte group and the storage-type dispatch.
#pragma once
#include "common.h"
#include "sde_hip.h"

// Grid-stride launches of 256-thread workgroups over n items.  A file keeps the cap it was tuned with; the grid is visible to callers
// (sde_depth_head_bias_blocks sizes a buffer by it), so the two are not merged.
constexpr int SDE_GRID_CAP_8K = 8192;       // nn, packnet
constexpr int SDE_GRID_CAP_16K = 16384;     // bts, google, motion, dense
static inline int sde_grid_for(long n, int cap) {
    const long nb = (n + 255) / 256;
    return (int)(nb < 1 ? 1 : nb > cap ? cap : nb);
}

// elements of the storage type in one 16-byte channel group (VecOf<T>::V of vec16.h, by dtype code)
static inline int sde_vec_elems(int dtype) { return SDE_IS16(dtype) ? 8 : 4; }

template <typename T> struct SdeDtypeOf;
template <> struct SdeDtypeOf<float> { static constexpr int value = SDE_F32; };
template <> struct SdeDtypeOf<bf16_t> { static constexpr int value = SDE_BF16; };
template <> struct SdeDtypeOf<half_t> { static constexpr int value = SDE_F16; };
template <typename T> struct SdeTag { typedef T type; static constexpr int size = sizeof(T); };

// The storage types a file instantiates its kernels for.  An entry point first refuses any other dtype,
//     SDE_CHECK_ARG(Types::has(dtype), "sde_x: unsupported dtype %d", dtype);
// and then writes each launch once:
//     Types::dispatch(dtype, [&](auto tag) {
//         typedef typename decltype(tag)::type T;
//         hipLaunchKernelGGL(x_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)x, (T*)y, n);
//     });
// dispatch instantiates the lambda for the listed types only and returns false, launching nothing, for a dtype outside the list.
// The list's order is the order in which a site's kernels are instantiated and so emitted into the code object (the left fold keeps it);
// each file lists its types in the order its kernels have always had, which keeps the code object byte for byte.
template <typename... Ts> struct SdeTypes {
    static bool has(int dtype) { return (... || (dtype == SdeDtypeOf<Ts>::value)); }
    template <typename F> static bool dispatch(int dtype, F&& f) { return (... || (dtype == SdeDtypeOf<Ts>::value ? (f(SdeTag<Ts>{}), true) : false)); }
};
