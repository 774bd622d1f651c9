// A sequence's depth fused into ONE truncated-signed-distance (TSDF) volume: every frame's depth is averaged into a voxel grid through the
// world-to-camera pose the predictor chains on the device, and the zero crossings of the grid are the surface.  The contract is written out
// in include/sde_hip.h.
//
// sde_pose_compose     C <- T * C for one rigid 4x4 transform, one workgroup of 64 threads: twelve of them read, a barrier, sixteen write.
// sde_tsdf_integrate   one voxel per thread, one grid-stride grid: centre -> camera (pinhole.h) -> nearest pixel -> the depth behind it through
//                      the index maps of sde_depth_present -> running average.  Voxels are independent: no atomics, the same bytes every run.
//                      Per touched voxel 12 B read (tsdf, weight, rgba) and 12 B written, 8 + 8 without colour; a voxel that is not kept
//                      costs no volume traffic, only the (cached) 4 B of depth when it projects into the picture.
// sde_tsdf_points      the zero crossings as the 16-byte records of sde_depth_cloud.  A tile is TILE consecutive voxels, one per thread, each with
//                      up to three crossings (towards its +x, +y, +z neighbour).  Stable compaction in three launches ordered on the stream:
//   points_count    crossings per tile: one __ballot per axis and wave, the wave sums added by thread 0 -> ws[tile];
//   points_scan     ONE workgroup walks the tile counts in chunks of TILE with a running carry (inclusive scan inside a wave by six __shfl_up
//                   steps, the wave totals through LDS): ws[tile] becomes the exclusive offset, count[0] the total;
//   points_scatter  the same decisions again, rank inside the wave = popcounts of the three ballots below the lane (+ the thread's own earlier
//                   axes), wave bases through LDS, record index = ws[tile] + wave base + rank; records at or beyond cap are not written.
// No workgroup waits for another, no atomics; the order is ascending voxel, then axis, run after run.  The scan is cloud.hip's, written again:
// that file's bytes stay what they are.
//
// Built with -ffp-contract=off: the projection, the average and the interpolation keep the operation order the header states, which
// hip/volume.py's host twins repeat bit for bit.
#include "common.h"
#include "pinhole.h"
#include "sde_hip.h"
#include "zbuf.h"

namespace {

constexpr int TILE = 256;
constexpr int MAX_BLOCKS = 2048;                 // 8 workgroups per compute unit; the grid-stride loops take the rest
constexpr int WAVES = TILE / 64;
constexpr int MAX_DIM = 1024;
constexpr long MAX_VOXELS = 1L << 30;

struct Grid {
    int nx, ny, nz;
    float ox, oy, oz, voxel;
};

struct IntegrateP {
    const float* pred;           // [ph][pw]
    const int* ymap;             // [H]
    const int* xmap;             // [W]
    const uint8_t* frame;        // [H][W][3] or null
    const float* K;              // [3][3]
    const float* C;              // [4][4]
    float* tsdf;                 // [nz][ny][nx]
    float* weight;               // [nz][ny][nx]
    uint32_t* rgba;              // [nz][ny][nx] or null
    Grid g;
    int H, W, ph, pw;
    float trunc, max_weight, min_depth, max_depth;
};

struct PointsP {
    const float* tsdf;
    const float* weight;
    const uint32_t* rgba;        // or null
    unsigned* ws;                // [ntiles]: counts, then exclusive offsets
    int* count;                  // [1]
    uint4* points;               // [cap]
    Grid g;
    size_t total, ntiles;
    unsigned cap;
    float min_weight;
};

__device__ __forceinline__ float centre(float o, int i, float voxel) { return o + ((float)i + 0.5f) * voxel; }

__device__ __forceinline__ void split(const Grid& g, size_t v, int& i, int& j, int& k) {
    const unsigned u = (unsigned)v, row = u / (unsigned)g.nx;                            // at most 2^30 voxels: 32-bit divisions
    i = (int)(u - row * (unsigned)g.nx);
    k = (int)(row / (unsigned)g.ny);
    j = (int)(row - (unsigned)k * (unsigned)g.ny);
}

__global__ void __launch_bounds__(64) pose_compose(const float* T, float* C) {
    const int t = threadIdx.x, r = t >> 2, c = t & 3;
    float v = 0.f;
    if (t < 12) {
        v = T[4 * r] * C[c] + T[4 * r + 1] * C[4 + c] + T[4 * r + 2] * C[8 + c];
        if (c == 3) v = v + T[4 * r + 3];
    } else if (t == 15) {
        v = 1.f;
    }
    __syncthreads();                                                                     // every read of C lies before every write
    if (t < 16) C[t] = v;
}

__global__ void __launch_bounds__(TILE) tsdf_integrate(IntegrateP p) {
    const size_t total = (size_t)p.g.nx * p.g.ny * p.g.nz;
    const Pinhole cam = pinhole_load(p.K);
    for (size_t v = (size_t)blockIdx.x * TILE + threadIdx.x; v < total; v += (size_t)gridDim.x * TILE) {
        int i, j, k;
        split(p.g, v, i, j, k);
        const float wx = centre(p.g.ox, i, p.g.voxel), wy = centre(p.g.oy, j, p.g.voxel), wz = centre(p.g.oz, k, p.g.voxel);
        float qx, qy, qz, X, Y;
        pinhole_move<4>(p.C, wx, wy, wz, p.C[3], p.C[7], p.C[11], qx, qy, qz);
        if (!(qz > 0.f && qz < INFINITY)) continue;                                      // a NaN fails the comparison
        pinhole_project(cam, qx, qy, qz, X, Y);
        int ix, iy;
        if (!nearest_pixel(X, Y, ix, iy)) continue;
        if (ix < 0 || ix >= p.W || iy < 0 || iy >= p.H) continue;
        const int my = p.ymap[iy], mx = p.xmap[ix];
        if (my < 0 || mx < 0) continue;
        const float d = p.pred[(size_t)my * p.pw + mx];
        if (!(fabsf(d) < INFINITY && p.min_depth < d && d <= p.max_depth)) continue;     // the cloud's rule
        const float sdf = d - qz;
        if (!(sdf >= -p.trunc)) continue;
        const float t = fminf(1.f, sdf / p.trunc);
        const float w0 = p.weight[v], t0 = p.tsdf[v];
        const float w1 = w0 + 1.f;
        p.tsdf[v] = (t0 * w0 + t) / w1;
        p.weight[v] = fminf(w1, p.max_weight);
        if (p.frame && p.rgba && sdf <= p.trunc) {
            const uint8_t* f = p.frame + ((size_t)iy * p.W + ix) * 3;
            const uint32_t c0 = p.rgba[v];
            uint32_t out = 0xff000000u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float c = ((float)((c0 >> (8 * ch)) & 255u) * w0 + (float)f[ch]) / w1;
                out |= ((uint32_t)(uint8_t)(c + 0.5f)) << (8 * ch);
            }
            p.rgba[v] = out;
        }
    }
}

// the crossings of voxel v towards its +x, +y, +z neighbours as bits 0..2; tv and the neighbours' values for the ones that are set
__device__ __forceinline__ unsigned crossings(const PointsP& p, size_t v, int i, int j, int k, float& tv, float tn[3]) {
    if (v >= p.total || !(p.weight[v] >= p.min_weight)) return 0u;
    tv = p.tsdf[v];
    const size_t step[3] = {(size_t)1, (size_t)p.g.nx, (size_t)p.g.nx * p.g.ny};
    const bool inside[3] = {i + 1 < p.g.nx, j + 1 < p.g.ny, k + 1 < p.g.nz};
    unsigned m = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!inside[a]) continue;
        const size_t n = v + step[a];
        if (!(p.weight[n] >= p.min_weight)) continue;
        tn[a] = p.tsdf[n];
        if ((tv < 0.f) != (tn[a] < 0.f)) m |= 1u << a;
    }
    return m;
}

__global__ void __launch_bounds__(TILE) points_count(PointsP p) {
    __shared__ unsigned wsum[WAVES];
    for (size_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {                 // the same trip count in every thread of the workgroup
        const size_t v = tile * TILE + threadIdx.x;
        int i = 0, j = 0, k = 0;
        if (v < p.total) split(p.g, v, i, j, k);
        float tv = 0.f, tn[3] = {0.f, 0.f, 0.f};
        const unsigned m = crossings(p, v, i, j, k, tv, tn);
        const unsigned n = (unsigned)(__popcll(__ballot(m & 1u)) + __popcll(__ballot(m & 2u)) + __popcll(__ballot(m & 4u)));
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) s += wsum[w];
            p.ws[tile] = s;
        }
        __syncthreads();                                                                 // wsum is written again by the next tile
    }
}

__global__ void __launch_bounds__(TILE) points_scan(unsigned* ws, int* count, size_t ntiles) {
    __shared__ unsigned wtot[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned carry = 0;                                          // crossings in front of this chunk: the same value in every thread
    for (size_t b0 = 0; b0 < ntiles; b0 += TILE) {
        const size_t b = b0 + threadIdx.x;
        const unsigned c = b < ntiles ? ws[b] : 0u;
        unsigned inc = c;                                        // inclusive scan over the wave
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned o = (unsigned)__shfl_up((int)inc, s, 64);
            if (lane >= s) inc += o;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        unsigned base = carry, total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) base += wtot[w];
            total += wtot[w];
        }
        if (b < ntiles) ws[b] = base + inc - c;                  // exclusive
        carry += total;
        __syncthreads();                                         // wtot is written again by the next chunk
    }
    if (threadIdx.x == 0) count[0] = carry > 0x7fffffffu ? 0x7fffffff : (int)carry;      // 3 * 2^30 crossings fit 32 unsigned bits, not a signed int
}

__global__ void __launch_bounds__(TILE) points_scatter(PointsP p) {
    __shared__ unsigned wsum[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (size_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const size_t v = tile * TILE + threadIdx.x;
        int i = 0, j = 0, k = 0;
        if (v < p.total) split(p.g, v, i, j, k);
        float tv = 0.f, tn[3] = {0.f, 0.f, 0.f};
        const unsigned m = crossings(p, v, i, j, k, tv, tn);
        const unsigned long long b0 = __ballot(m & 1u), b1 = __ballot(m & 2u), b2 = __ballot(m & 4u);
        if (lane == 0) wsum[wave] = (unsigned)(__popcll(b0) + __popcll(b1) + __popcll(b2));
        __syncthreads();
        if (m) {
            unsigned at = p.ws[tile] + (unsigned)(__popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below));
            for (int w = 0; w < wave; ++w) at += wsum[w];
            const float cx = centre(p.g.ox, i, p.g.voxel), cy = centre(p.g.oy, j, p.g.voxel), cz = centre(p.g.oz, k, p.g.voxel);
            const size_t step[3] = {(size_t)1, (size_t)p.g.nx, (size_t)p.g.nx * p.g.ny};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!(m & (1u << a))) continue;
                if (at < p.cap) {
                    const float f = tv / (tv - tn[a]);
                    const float along = f * p.g.voxel;
                    const float x = a == 0 ? cx + along : cx, y = a == 1 ? cy + along : cy, z = a == 2 ? cz + along : cz;
                    uint32_t rgba = 0xff000000u;
                    if (p.rgba) rgba = (p.rgba[f < 0.5f ? v : v + step[a]] & 0x00ffffffu) | 0xff000000u;
                    p.points[at] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), rgba);
                }
                ++at;
            }
        }
        __syncthreads();                                                                 // wsum is written again by the next tile
    }
}

bool dims_ok(int nx, int ny, int nz) {
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= MAX_DIM && ny <= MAX_DIM && nz <= MAX_DIM && (long)nx * ny * nz <= MAX_VOXELS;
}

unsigned blocks_for(size_t n) { return zbuf_blocks(n, TILE, MAX_BLOCKS); }

}  // namespace

extern "C" {

int sde_pose_compose(const float* T, float* C, sde_stream_t stream) {
    SDE_CHECK_ARG(T && C, "sde_pose_compose: null pointer");
    hipLaunchKernelGGL(pose_compose, dim3(1), dim3(64), 0, (hipStream_t)stream, T, C);
    SDE_CHECK_LAUNCH("sde_pose_compose");
    return SDE_OK;
}

int sde_tsdf_integrate(const float* pred, int ph, int pw, const int* ymap, const int* xmap, int H, int W, const uint8_t* frame, const float* K,
                       const float* C, const float* origin, float voxel, float trunc, float max_weight, float min_depth, float max_depth,
                       float* tsdf, float* weight, uint8_t* rgba, int nx, int ny, int nz, sde_stream_t stream) {
    SDE_CHECK_ARG(H > 0 && W > 0 && ph > 0 && pw > 0, "sde_tsdf_integrate: bad shape (%dx%d -> %dx%d)", ph, pw, H, W);
    SDE_CHECK_ARG((long)ph * pw <= 0x7fffffffL && (long)H * W <= 0x7fffffffL, "sde_tsdf_integrate: map too large");
    SDE_CHECK_ARG(dims_ok(nx, ny, nz), "sde_tsdf_integrate: every dimension must lie in [1, %d] and their product be at most 2^30 (%d x %d x %d)", MAX_DIM, nx,
                  ny, nz);
    SDE_CHECK_ARG(voxel > 0.f && trunc > 0.f && max_weight > 0.f, "sde_tsdf_integrate: voxel, trunc and max_weight must be positive (%g, %g, %g)",
                  (double)voxel, (double)trunc, (double)max_weight);                                     // a NaN fails the comparison
    SDE_CHECK_ARG(min_depth < max_depth, "sde_tsdf_integrate: min_depth must lie below max_depth (%g, %g)", (double)min_depth, (double)max_depth);
    SDE_CHECK_ARG(pred && ymap && xmap && K && C && origin && tsdf && weight, "sde_tsdf_integrate: null pointer");
    SDE_CHECK_ARG(((uintptr_t)rgba & 3) == 0, "sde_tsdf_integrate: rgba must be 4-byte aligned");
    IntegrateP p{pred, ymap, xmap, frame, K, C, tsdf, weight, (uint32_t*)rgba, Grid{nx, ny, nz, origin[0], origin[1], origin[2], voxel},
                 H, W, ph, pw, trunc, max_weight, min_depth, max_depth};
    hipLaunchKernelGGL(tsdf_integrate, dim3(blocks_for((size_t)nx * ny * nz)), dim3(TILE), 0, (hipStream_t)stream, p);
    SDE_CHECK_LAUNCH("sde_tsdf_integrate");
    return SDE_OK;
}

size_t sde_tsdf_points_ws_bytes(int nx, int ny, int nz) {
    if (!dims_ok(nx, ny, nz)) return 0;
    return (size_t)(((long)nx * ny * nz + TILE - 1) / TILE) * sizeof(unsigned);
}

int sde_tsdf_points(const float* tsdf, const float* weight, const uint8_t* rgba, int nx, int ny, int nz, const float* origin, float voxel,
                    float min_weight, void* workspace, size_t workspace_bytes, void* points, long cap, int* count, sde_stream_t stream) {
    SDE_CHECK_ARG(dims_ok(nx, ny, nz), "sde_tsdf_points: every dimension must lie in [1, %d] and their product be at most 2^30 (%d x %d x %d)", MAX_DIM, nx, ny,
                  nz);
    SDE_CHECK_ARG(voxel > 0.f, "sde_tsdf_points: voxel must be positive (%g)", (double)voxel);
    SDE_CHECK_ARG(min_weight >= 1.f, "sde_tsdf_points: min_weight must be at least 1 (%g)", (double)min_weight);
    SDE_CHECK_ARG(cap >= 1 && cap <= 0x7fffffffL, "sde_tsdf_points: cap must lie in [1, 2^31) (%ld)", cap);
    SDE_CHECK_ARG(tsdf && weight && origin && points && count, "sde_tsdf_points: null pointer");
    SDE_CHECK_ARG(((uintptr_t)points & 15) == 0, "sde_tsdf_points: points must be 16-byte aligned");
    SDE_CHECK_ARG(((uintptr_t)rgba & 3) == 0, "sde_tsdf_points: rgba must be 4-byte aligned");
    const size_t need = sde_tsdf_points_ws_bytes(nx, ny, nz);
    SDE_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
                  "sde_tsdf_points: workspace of %zu bytes, sde_tsdf_points_ws_bytes asks for %zu", workspace ? workspace_bytes : (size_t)0, need);
    PointsP p{tsdf, weight, (const uint32_t*)rgba, (unsigned*)workspace, count, (uint4*)points, Grid{nx, ny, nz, origin[0], origin[1], origin[2], voxel},
              (size_t)nx * ny * nz, need / sizeof(unsigned), (unsigned)cap, min_weight};
    const unsigned grid = (unsigned)(p.ntiles < (size_t)MAX_BLOCKS ? p.ntiles : (size_t)MAX_BLOCKS);
    hipLaunchKernelGGL(points_count, dim3(grid), dim3(TILE), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(points_scan, dim3(1), dim3(TILE), 0, (hipStream_t)stream, p.ws, count, p.ntiles);
    hipLaunchKernelGGL(points_scatter, dim3(grid), dim3(TILE), 0, (hipStream_t)stream, p);
    SDE_CHECK_LAUNCH("sde_tsdf_points");
    return SDE_OK;
}

}  // extern "C"
