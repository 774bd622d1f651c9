// Deterministic reductions of the loss kernels (included by common.h): wave and block sums, the strided walk over a slab of per-workgroup
// partials, and the arrival count by which the workgroup that finishes last completes a reduction.  Additions only -- every `* scale` stays at its
// call site -- so the helpers mean the same in the -ffp-contract=off objects and in the default ones.  See DESIGN.md section 27.
#pragma once
#include <hip/hip_runtime.h>

// Sum over the 64 lanes of a wave, returned in every lane.  DPP adds instead of six __shfl_xor steps (ds_bpermute_b32: an LDS-crossbar round
// trip each): quad swaps, row half-mirror and mirror give every lane its 16-lane row sum; row_bcast15 / row_bcast31 chain the four rows into
// lane 63, which v_readlane broadcasts.  Fixed order: deterministic.
__device__ __forceinline__ float sde_wave_sum(float v) {
    auto step = [](float x, auto CTRL, auto ROWS) {
        const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(CTRL)::value, decltype(ROWS)::value, 0xf, false);
        return x + __builtin_bit_cast(float, moved);
    };
    struct C_B1 { enum { value = 0xB1 }; }; struct C_4E { enum { value = 0x4E }; }; struct C_141 { enum { value = 0x141 }; };
    struct C_140 { enum { value = 0x140 }; }; struct C_142 { enum { value = 0x142 }; }; struct C_143 { enum { value = 0x143 }; };
    struct R_F { enum { value = 0xf }; }; struct R_A { enum { value = 0xa }; }; struct R_C { enum { value = 0xc }; };
    v = step(v, C_B1{}, R_F{});      // quad_perm [1,0,3,2]
    v = step(v, C_4E{}, R_F{});      // quad_perm [2,3,0,1]
    v = step(v, C_141{}, R_F{});     // row_half_mirror
    v = step(v, C_140{}, R_F{});     // row_mirror: every lane holds its row's sum
    v = step(v, C_142{}, R_A{});     // row_bcast15 into rows 1 and 3
    v = step(v, C_143{}, R_C{});     // row_bcast31 into rows 2 and 3: lane 63 holds the wave's sum
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// ---- block sums -------------------------------------------------------------------------------------------------------------------------------
// Barrier contract of sde_block_sums and sde_block_sum: every thread of the block calls; the block is a multiple of 64 threads, at most 1024.  A call
// opens with a barrier and has one more between the wave leaders' writes to `red` and the reads.  The opening barrier is what lets a call follow
// another call on the same `red` (or any earlier use of it) with no barrier from the caller: the previous call's readers are through before a
// leader overwrites their slots.  A call does NOT close with a barrier: whoever reads `out` in another thread than the one that wrote it puts one.

// Sums of NV values over the block: waves added in wave order, threads 0..NV-1 write out[0..NV) (LDS or global).  `red` >= NV floats per wave.
// NW: the block's wave count where the caller knows it at compile time (the loop over the waves unrolls and its LDS loads issue together: 1 us on
// a pass of 7168 workgroups); 0 reads it from blockDim.
template <int NV, int NW = 0>
__device__ __forceinline__ void sde_block_sums(float (&v)[NV], float* red, float* out) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = sde_wave_sum(v[i]);
    const int tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
    const int nw = NW ? NW : (blockDim.x * blockDim.y * blockDim.z + 63) >> 6;
    __syncthreads();
    if ((tid & 63) == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) red[(tid >> 6) * NV + i] = v[i];
    __syncthreads();
    if (tid < NV) {
        float r = red[tid];
#pragma unroll
        for (int w = 1; w < nw; ++w) r += red[w * NV + tid];
        out[tid] = r;
    }
}

// The scalar convenience: result valid in thread 0.  `red` >= 16 floats.
__device__ __forceinline__ float sde_block_sum(float v, float* red) {
    v = sde_wave_sum(v);
    const int tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
    const int nw = (blockDim.x * blockDim.y * blockDim.z + 63) >> 6;
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float r = 0.f;
    if (tid == 0)
        for (int i = 0; i < nw; ++i) r += red[i];
    return r;
}

// ---- partial slabs ----------------------------------------------------------------------------------------------------------------------------
// acc[k] += partial[(first + i) * pitch + k] for i = tid, tid + STRIDE, ... < count and k < NV: thread `tid`'s share of a slab of `count` partials of NV
// interleaved values.  STRIDE 64: one wave per slab; 256: one workgroup.  The caller zeroes acc and then sums the shares (wave or block sum).
template <int NV, int STRIDE>
__device__ __forceinline__ void sde_partial_walk(float* acc, const float* __restrict__ partial, long first, int count, int tid, int pitch = NV) {
    for (int i = tid; i < count; i += STRIDE)
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += partial[(first + i) * pitch + k];
}

// v[lane] for lane < NV (else 0) without indexing the register array by a runtime value
template <int NV>
__device__ __forceinline__ float sde_lane_pick(const float (&v)[NV], int lane) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s = lane == i ? v[i] : s;
    return s;
}

// ---- the workgroup that arrives last finishes the job -----------------------------------------------------------------------------------------
__device__ __forceinline__ float ld_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Called by every thread of each of `count` workgroups (1-D blocks), after thread 0 has published the workgroup's values with agent-scope stores.  True, in every
// thread, in the workgroup that arrives last; that one reads what the others published with ld_agent.  Leaves *ticket at zero, so launches that count
// on the same int must be ordered on one stream.
// Why this is sufficient.  Publisher: the release fence orders thread 0's agent-scope stores before its fetch_add.  The fetch_adds
// on the ticket form one modification order, each an acquire-release read-modify-write, so the one that reads count - 1 is ordered after every
// earlier arriver's fence and with it after their stores.  The barrier hands that order from thread 0 to the rest of its workgroup, and the second
// fence (an acquire, in every thread of the last workgroup) keeps the loads that follow from being satisfied by anything older.  Nobody counts
// after the last arriver, and the next launch on the stream starts after this one, so the reset needs no further ordering.  The fences are
// one-sided on purpose: a full __threadfence() in every wave of the last workgroup writes the L2 back once per wave (+0.5 us at 256 threads,
// +2.6 us at 1024, profiles/loss_reduce_ab.txt).
__device__ __forceinline__ bool sde_arrive_last(int* ticket, int count) {
    __shared__ int last;
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        last = (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == count - 1);
        if (last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return true;
}
