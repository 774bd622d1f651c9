// The z-buffer of the forward-projecting kernels (lidar.hip, temporal.hip), ONE definition: a map of float bit patterns that starts at +inf and
// takes the minimum of whatever lands.  Depths that reach it are positive finite floats, which order like their bit patterns, so the unsigned
// minimum is the float minimum; a minimum does not depend on arrival order: the same bits run after run.
#pragma once
#include "common.h"

namespace {

constexpr unsigned ZBUF_EMPTY = 0x7f800000u;     // +inf: above every depth that is kept

template <int TILE>
__global__ void __launch_bounds__(TILE) zbuf_fill(unsigned* __restrict__ zbuf, size_t n) {
    for (size_t i = (size_t)blockIdx.x * TILE + threadIdx.x; i < n; i += (size_t)gridDim.x * TILE) zbuf[i] = ZBUF_EMPTY;
}

// ONE no-return atomic on the entry's bits
__device__ __forceinline__ void zbuf_min(unsigned* at, float depth) { atomicMin(at, __float_as_uint(depth)); }

// workgroups of `tile` threads for n elements, at most `cap`: the grid-stride loops take the rest
inline unsigned zbuf_blocks(size_t n, int tile, int cap) { return (unsigned)(n / tile >= (size_t)cap ? cap : (n + tile - 1) / tile); }

}  // namespace
