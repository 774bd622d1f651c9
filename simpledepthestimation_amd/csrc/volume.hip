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
// sde_tsdf_mesh        the same crossings connected into triangles by surface nets (one vertex per cell with a crossing, one quad per crossing
//                      edge): four launches, described in front of its kernels below.
// sde_tsdf_render      the volume seen from a camera pose (depth, normal, colour) by ray casting: one launch, one thread per pixel, described in
//                      front of its kernel below.
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

// ---- sde_tsdf_mesh: surface nets -------------------------------------------------------------------------------------------------------------------
// One thread per voxel, which stands for the cell whose lowest corner it is AND for its own three edges.  Four launches:
//   mesh_count     the 8 corners of the cell (weight, and tsdf where valid: plain loads, neighbours in x share cache lines, the rows above come
//                  from L2) -> the 12 edge bits; cells with a vertex and quads per tile -> ws_v[tile], ws_q[tile].  A quad belongs to the voxel
//                  its edge starts at, and an edge with all four cells around it is edge 0, 4 or 8 of that voxel's own cell: one mask serves both;
//   mesh_scan      both lists by one workgroup with a running carry, 8 rows of 256 counts per step; count[0] = vertices, count[1] = 2 * quads;
//   mesh_vertices  the same masks, rank = ws_v[tile] + wave base + popcount below the lane: map[cell] = rank, and the record where rank < cap;
//   mesh_faces     crossings() of the voxel's own edges as in points_scatter, the four vertex numbers from map, two triangles per quad.
// map is written for every cell with a vertex and read only for cells around a crossing edge, which have one: it needs no clearing.
struct MeshP {
    PointsP pt;                  // the volume; ws = vertex counts / offsets per tile, points = the vertices, cap = cap_vertices, count [2]
    unsigned* ws_q;              // [ntiles] quads per tile, then exclusive offsets
    unsigned* map;               // [total] cell -> vertex number
    int* faces;                  // [cap_faces][3]
    size_t cap_faces;
};

// corner c = di + 2 dj + 4 dk of a cell; edge e = 4 a + (db + 2 dc) runs from corner edge_lo(a, db, dc) along axis a
__device__ __forceinline__ constexpr int edge_lo(int a, int db, int dc) { return a == 0 ? 2 * db + 4 * dc : a == 1 ? db + 4 * dc : db + 2 * dc; }

// the crossing edges of the cell at voxel v as bits 0..11 (0: no such cell); t: tsdf of the valid corners.  The tests are those of crossings().
__device__ __forceinline__ unsigned cell_edges(const PointsP& p, size_t v, int i, int j, int k, float t[8]) {
    if (v >= p.total || i + 1 >= p.g.nx || j + 1 >= p.g.ny || k + 1 >= p.g.nz) return 0u;
    const size_t sy = (size_t)p.g.nx, sz = (size_t)p.g.nx * p.g.ny;
    unsigned valid = 0u, neg = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const size_t n = v + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz;
        if (!(p.weight[n] >= p.min_weight)) continue;
        valid |= 1u << c;
        t[c] = p.tsdf[n];
        if (t[c] < 0.f) neg |= 1u << c;
    }
    unsigned m = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int lo = edge_lo(a, e & 1, e >> 1), hi = lo + (1 << a);
            if (((valid >> lo) & (valid >> hi) & 1u) && (((neg >> lo) ^ (neg >> hi)) & 1u)) m |= 1u << (4 * a + e);
        }
    return m;
}

// of the voxel's own crossings (bits 0..2 = axes), those with four cells around the edge
__device__ __forceinline__ unsigned face_mask(const Grid& g, unsigned mc, int i, int j, int k) {
    const bool bx = i >= 1 && i <= g.nx - 2, by = j >= 1 && j <= g.ny - 2, bz = k >= 1 && k <= g.nz - 2;
    return mc & ((by && bz ? 1u : 0u) | (bx && bz ? 2u : 0u) | (bx && by ? 4u : 0u));
}

__global__ void __launch_bounds__(TILE) mesh_count(MeshP p) {
    __shared__ unsigned wsum[2][WAVES];
    for (size_t tile = blockIdx.x; tile < p.pt.ntiles; tile += gridDim.x) {             // the same trip count in every thread of the workgroup
        const size_t v = tile * TILE + threadIdx.x;
        int i = 0, j = 0, k = 0;
        if (v < p.pt.total) split(p.pt.g, v, i, j, k);
        float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const unsigned m = cell_edges(p.pt, v, i, j, k, t);
        const unsigned fb = face_mask(p.pt.g, (m & 1u) | ((m >> 3) & 2u) | ((m >> 6) & 4u), i, j, k);
        const unsigned nv = (unsigned)__popcll(__ballot(m != 0u));
        const unsigned nq = (unsigned)(__popcll(__ballot(fb & 1u)) + __popcll(__ballot(fb & 2u)) + __popcll(__ballot(fb & 4u)));
        if ((threadIdx.x & 63) == 0) {
            wsum[0][threadIdx.x >> 6] = nv;
            wsum[1][threadIdx.x >> 6] = nq;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) s += wsum[threadIdx.x][w];
            (threadIdx.x == 0 ? p.pt.ws : p.ws_q)[tile] = s;
        }
        __syncthreads();                                                                 // wsum is written again by the next tile
    }
}

// points_scan's walk with a running carry, but a chunk is SCAN_ROWS rows of TILE counts of BOTH lists held in registers: sixteen independent
// loads, their wave scans, ONE pair of barriers.  The walk is serial and every chunk costs a round trip to memory: 2 * ntiles / TILE of them
// (a 256 x 256 x 128 grid: 256) took more time than the other three launches together; this way they are ntiles / (SCAN_ROWS * TILE) (16).
constexpr int SCAN_ROWS = 8;

__global__ void __launch_bounds__(TILE) mesh_scan(unsigned* ws_v, unsigned* ws_q, int* count, size_t ntiles) {
    __shared__ unsigned wtot[2][SCAN_ROWS][WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* const ws[2] = {ws_v, ws_q};
    unsigned carry[2] = {0u, 0u};                                // entries in front of this chunk: the same values in every thread
    for (size_t b0 = 0; b0 < ntiles; b0 += (size_t)SCAN_ROWS * TILE) {
        unsigned c[2][SCAN_ROWS], inc[2][SCAN_ROWS];
#pragma unroll
        for (int l = 0; l < 2; ++l)
#pragma unroll
            for (int r = 0; r < SCAN_ROWS; ++r) {
                const size_t b = b0 + (size_t)r * TILE + threadIdx.x;
                inc[l][r] = c[l][r] = b < ntiles ? ws[l][b] : 0u;
            }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {                       // inclusive scans over the wave; the step outermost: sixteen shuffles in flight
            unsigned o[2][SCAN_ROWS];
#pragma unroll
            for (int l = 0; l < 2; ++l)
#pragma unroll
                for (int r = 0; r < SCAN_ROWS; ++r) o[l][r] = (unsigned)__shfl_up((int)inc[l][r], s, 64);
#pragma unroll
            for (int l = 0; l < 2; ++l)
#pragma unroll
                for (int r = 0; r < SCAN_ROWS; ++r)
                    if (lane >= s) inc[l][r] += o[l][r];
        }
        if (lane == 63) {
#pragma unroll
            for (int l = 0; l < 2; ++l)
#pragma unroll
                for (int r = 0; r < SCAN_ROWS; ++r) wtot[l][r][wave] = inc[l][r];
        }
        __syncthreads();
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            unsigned base = carry[l];
#pragma unroll
            for (int r = 0; r < SCAN_ROWS; ++r) {
                unsigned mine = base;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) {
                    if (w < wave) mine += wtot[l][r][w];
                    base += wtot[l][r][w];
                }
                const size_t b = b0 + (size_t)r * TILE + threadIdx.x;
                if (b < ntiles) ws[l][b] = mine + inc[l][r] - c[l][r];               // exclusive
            }
            carry[l] = base;
        }
        __syncthreads();                                         // wtot is written again by the next chunk
    }
    if (threadIdx.x == 0) {
        count[0] = (int)carry[0];                                // at most 2^30 cells
        count[1] = carry[1] > 0x3fffffffu ? 0x7fffffff : (int)(2u * carry[1]);           // at most 3 * 2^30 quads: the offsets stay in quads
    }
}

__global__ void __launch_bounds__(TILE) mesh_vertices(MeshP p) {
    __shared__ unsigned wsum[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const Grid& g = p.pt.g;
    const size_t step[3] = {(size_t)1, (size_t)g.nx, (size_t)g.nx * g.ny};
    for (size_t tile = blockIdx.x; tile < p.pt.ntiles; tile += gridDim.x) {
        const size_t v = tile * TILE + threadIdx.x;
        int i = 0, j = 0, k = 0;
        if (v < p.pt.total) split(g, v, i, j, k);
        float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const unsigned m = cell_edges(p.pt, v, i, j, k, t);
        const unsigned long long has = __ballot(m != 0u);
        if (lane == 0) wsum[wave] = (unsigned)__popcll(has);
        __syncthreads();
        if (m) {
            unsigned at = p.pt.ws[tile] + (unsigned)__popcll(has & below);
            for (int w = 0; w < wave; ++w) at += wsum[w];
            p.map[v] = at;
            if (at < p.pt.cap) {
                const float cx[2] = {centre(g.ox, i, g.voxel), centre(g.ox, i + 1, g.voxel)};
                const float cy[2] = {centre(g.oy, j, g.voxel), centre(g.oy, j + 1, g.voxel)};
                const float cz[2] = {centre(g.oz, k, g.voxel), centre(g.oz, k + 1, g.voxel)};
                uint32_t col[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};                    // the corners' colours: eight independent loads, not up to twelve in a chain
                if (p.pt.rgba) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) col[c] = p.pt.rgba[v + (c & 1) * step[0] + ((c >> 1) & 1) * step[1] + (c >> 2) * step[2]];
                }
                float sx = 0.f, sy = 0.f, sz = 0.f;
                unsigned sr = 0u, sg = 0u, sb = 0u, n = 0u;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (!(m & (1u << (4 * a + e)))) continue;
                        const int lo = edge_lo(a, e & 1, e >> 1), hi = lo + (1 << a);
                        const float f = t[lo] / (t[lo] - t[hi]);
                        const float along = f * g.voxel;
                        const float x = cx[lo & 1], y = cy[(lo >> 1) & 1], z = cz[lo >> 2];
                        sx = sx + (a == 0 ? x + along : x);
                        sy = sy + (a == 1 ? y + along : y);
                        sz = sz + (a == 2 ? z + along : z);
                        const uint32_t rgb = f < 0.5f ? col[lo] : col[hi];
                        sr += rgb & 255u;
                        sg += (rgb >> 8) & 255u;
                        sb += (rgb >> 16) & 255u;
                        ++n;
                    }
                const float fm = (float)n;
                const uint32_t rgba = 0xff000000u | (uint32_t)(uint8_t)((float)sr / fm + 0.5f) | ((uint32_t)(uint8_t)((float)sg / fm + 0.5f) << 8) |
                                      ((uint32_t)(uint8_t)((float)sb / fm + 0.5f) << 16);
                p.pt.points[at] = make_uint4(__float_as_uint(sx / fm), __float_as_uint(sy / fm), __float_as_uint(sz / fm), rgba);
            }
        }
        __syncthreads();                                                                 // wsum is written again by the next tile
    }
}

__global__ void __launch_bounds__(TILE) mesh_faces(MeshP p) {
    __shared__ unsigned wsum[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const Grid& g = p.pt.g;
    const size_t step[3] = {(size_t)1, (size_t)g.nx, (size_t)g.nx * g.ny};
    for (size_t tile = blockIdx.x; tile < p.pt.ntiles; tile += gridDim.x) {
        const size_t v = tile * TILE + threadIdx.x;
        int i = 0, j = 0, k = 0;
        if (v < p.pt.total) split(g, v, i, j, k);
        float tv = 0.f, tn[3] = {0.f, 0.f, 0.f};
        const unsigned m = face_mask(g, crossings(p.pt, v, i, j, k, tv, tn), i, j, k);
        const unsigned long long b0 = __ballot(m & 1u), b1 = __ballot(m & 2u), b2 = __ballot(m & 4u);
        if (lane == 0) wsum[wave] = (unsigned)(__popcll(b0) + __popcll(b1) + __popcll(b2));
        __syncthreads();
        if (m) {
            unsigned at = p.ws_q[tile] + (unsigned)(__popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below));
            for (int w = 0; w < wave; ++w) at += wsum[w];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!(m & (1u << a))) continue;
                const size_t sb = step[a == 0 ? 1 : 0], sc = step[a == 2 ? 1 : 2];       // b < c, the other two axes; face_mask: both >= 1 here
                const size_t tri = 2 * (size_t)at;
                if (tri < p.cap_faces) {
                    const int q0 = (int)p.map[v - sb - sc], q1 = (int)p.map[v - sc], q2 = (int)p.map[v], q3 = (int)p.map[v - sb];
                    const bool keep = (tv < 0.f) != (a == 1);
                    const int p1 = keep ? q1 : q3, p3 = keep ? q3 : q1;
                    int* f = p.faces + 3 * tri;
                    f[0] = q0, f[1] = p1, f[2] = q2;
                    if (tri + 1 < p.cap_faces) f[3] = q0, f[4] = q2, f[5] = p3;
                }
                ++at;
            }
        }
        __syncthreads();                                                                 // wsum is written again by the next tile
    }
}

// ---- sde_tsdf_render: ray casting -------------------------------------------------------------------------------------------------------------------
// One thread per pixel, one launch.  A wave is an 8 x 8 pixel tile, a workgroup four of them side by side (32 x 8 pixels): neighbouring rays walk
// neighbouring cells, so the eight corner loads of a sample fall into few cache lines per wave.  Per sample 8 weights and 8 tsdf values, all
// sixteen loads issued before the first is used; the march is a chain of such round trips to the cache, and the kernel is bound by their latency.
//
// Skipping.  The result is defined by the full march over i = 0 .. n-1, but only VALID samples can matter, and a valid sample has
// 0 <= g_r < n_r - 1 on every axis.  In exact arithmetic g_r is affine in s: g_r(s) = s * a_r + c_r with a_r = D_r / voxel,
// c_r = (O_r - origin_r) / voxel - 0.5, D_r = R_0r rx + R_1r ry + R_2r, O_r = -(R_0r t_0 + R_1r t_1 + R_2r t_2), which fp64 gives from the fp32
// inputs with a relative error of 2^-50.  The fp32 value the march computes differs from it, counted to first order with EPS = 2^-24:
//   p_k = s ray_k, d_k = p_k - t_k, R_kr d_k, two sums:      |w_r - exact| <= EPS sum_k |R_kr| (5 |p_k| + 4 |t_k|) <= 5 EPS (A_r |s| + B_r),
//   (w - o), / voxel, - 0.5 on a result in [0, 1024):        + 3 EPS (|g| + 0.5) <= 2e-4 grid units,
// with A_r = sum_k |R_kr ray_k|, B_r = sum_k |R_kr t_k|.  The box is widened by m_r = 8 EPS (A_r smax + B_r) / voxel + 1e-3, smax = |near| + n step:
// beyond twice the first-order count.  s_i itself is two roundings from near + i step, at most 2 EPS smax: the interval in s is widened by
// 4 EPS smax before it becomes an index range, and that range by one index on either side.  Every sample outside the range is invalid whatever
// the memory holds, the sample in front of the range among them: the march starts at its first index with prev cleared and ends at its last.
constexpr int RENDER_TW = 32, RENDER_TH = 8;      // pixels per workgroup: four 8 x 8 waves side by side
constexpr int MAX_SAMPLES = 65536;
constexpr int MAX_PICTURE = 32768;                // pixels along either side

struct RenderP {
    const float* tsdf;
    const float* weight;
    const uint32_t* rgba;        // or null
    const float* K;              // [3][3]
    const float* C;              // [4][4]
    float* depth;                // [H][W]
    float* normal;               // [H][W][3] or null
    uint32_t* picture;           // [H][W] or null
    Grid g;
    int H, W, n;
    float near, step, min_weight;
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < INFINITY; }       // a NaN fails the comparison

__device__ __forceinline__ void render_miss(const RenderP& p, size_t px) {
    p.depth[px] = 0.f;
    if (p.normal) p.normal[3 * px] = 0.f, p.normal[3 * px + 1] = 0.f, p.normal[3 * px + 2] = 0.f;
    if (p.picture) p.picture[px] = 0u;
}

__global__ void __launch_bounds__(RENDER_TW * RENDER_TH) tsdf_render(RenderP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * RENDER_TW + wave * 8 + (lane & 7), v = blockIdx.y * RENDER_TH + (lane >> 3);
    if (u >= p.W || v >= p.H) return;
    const size_t px = (size_t)v * p.W + u;
    const Grid& g = p.g;
    float R[3][3], t[3];
    bool ok = g.nx >= 2 && g.ny >= 2 && g.nz >= 2;                                        // a dimension of 1: no cells
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = p.C[4 * r + c], ok = ok && finite_f(R[r][c]);
        t[r] = p.C[4 * r + 3], ok = ok && finite_f(t[r]);
    }
    const Pinhole cam = pinhole_load(p.K);
    ok = ok && finite_f(cam.fx) && finite_f(cam.cx) && finite_f(cam.fy) && finite_f(cam.cy);
    const float rx = cam.k00 * (float)u + cam.k02, ry = cam.k11 * (float)v + cam.k12;
    // a ray component that is not finite makes d_0 or d_1, and with it every w_r, not finite at every s: no sample is valid
    if (!ok || !finite_f(rx) || !finite_f(ry)) { render_miss(p, px); return; }

    const float o[3] = {g.ox, g.oy, g.oz};
    const int dim[3] = {g.nx, g.ny, g.nz};
    const double ray[3] = {(double)rx, (double)ry, 1.0};
    const double smax = fabs((double)p.near) + (double)p.n * (double)p.step, eps = 1.0 / 16777216.0, voxel = (double)g.voxel;
    double slo = -(double)INFINITY, shi = (double)INFINITY;
    bool empty = false;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double D = 0.0, O = 0.0, A = 0.0, B = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double Rk = (double)R[k][r];
            D += Rk * ray[k], O -= Rk * (double)t[k], A += fabs(Rk * ray[k]), B += fabs(Rk * (double)t[k]);
        }
        const double a = D / voxel, c = (O - (double)o[r]) / voxel - 0.5, m = 8.0 * eps * (A * smax + B) / voxel + 1e-3;
        const double lo = -m - c, hi = (double)(dim[r] - 1) + m - c;                   // lo <= s * a <= hi
        if (a == 0.0) {
            if (!(lo <= 0.0 && 0.0 <= hi)) empty = true;
        } else {
            const double s0 = lo / a, s1 = hi / a;
            slo = fmax(slo, fmin(s0, s1)), shi = fmin(shi, fmax(s0, s1));
        }
    }
    const double ds = 4.0 * eps * smax;
    const double flo = floor((slo - ds - (double)p.near) / (double)p.step) - 1.0, fhi = ceil((shi + ds - (double)p.near) / (double)p.step) + 1.0;
    if (empty || !(flo <= fhi) || !(fhi >= 0.0) || !(flo <= (double)(p.n - 1))) { render_miss(p, px); return; }
    const int i0 = flo > 0.0 ? (int)flo : 0, i1 = fhi < (double)(p.n - 1) ? (int)fhi : p.n - 1;

    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * g.ny;
    const float top[3] = {(float)(g.nx - 2), (float)(g.ny - 2), (float)(g.nz - 2)};
    bool prev = false;
    float tp = 0.f;
    for (int i = i0; i <= i1; ++i) {
        const float s = p.near + (float)i * p.step;
        const float d0 = s * rx - t[0], d1 = s * ry - t[1], d2 = s - t[2];
        float gr[3], b[3];
        bool valid = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float w = R[0][r] * d0 + R[1][r] * d1 + R[2][r] * d2;
            gr[r] = (w - o[r]) / g.voxel - 0.5f;
            b[r] = floorf(gr[r]);
            valid = valid && finite_f(gr[r]) && b[r] >= 0.f && b[r] <= top[r];
        }
        if (!valid) { prev = false; continue; }
        const float fx = gr[0] - b[0], fy = gr[1] - b[1], fz = gr[2] - b[2];
        const int bx = (int)b[0], by = (int)b[1], bz = (int)b[2];
        const size_t base = (size_t)bz * sz + (size_t)by * sy + (size_t)bx;
        float wt[8], T[8];                                                               // corner c = dx + 2 dy + 4 dz
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const size_t at = base + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz;
            wt[c] = p.weight[at];
            T[c] = p.tsdf[at];
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) valid = valid && wt[c] >= p.min_weight;
        if (!valid) { prev = false; continue; }
        float cz[4], e[2];                                                               // c_zy at 2 z + y
#pragma unroll
        for (int q = 0; q < 4; ++q) cz[q] = T[2 * q] + fx * (T[2 * q + 1] - T[2 * q]);
        e[0] = cz[0] + fy * (cz[1] - cz[0]);
        e[1] = cz[2] + fy * (cz[3] - cz[2]);
        const float ti = e[0] + fz * (e[1] - e[0]);
        if (prev && tp > 0.f && ti <= 0.f) {
            const float sp = p.near + (float)(i - 1) * p.step;
            p.depth[px] = sp + p.step * (tp / (tp - ti));
            if (p.normal) {
                float X[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) X[q] = T[2 * q + 1] - T[2 * q];
                const float x0 = X[0] + fy * (X[1] - X[0]), x1 = X[2] + fy * (X[3] - X[2]);
                const float gx = x0 + fz * (x1 - x0);
                const float y0 = cz[1] - cz[0], y1 = cz[3] - cz[2];
                const float gy = y0 + fz * (y1 - y0);
                const float gz = e[1] - e[0];
                const float len = sqrtf(gx * gx + gy * gy + gz * gz);
                const bool unit = len > 0.f && len < INFINITY;
#pragma unroll
                for (int r = 0; r < 3; ++r) p.normal[3 * px + r] = unit ? (R[r][0] * gx + R[r][1] * gy + R[r][2] * gz) / len : 0.f;
            }
            if (p.picture)
                p.picture[px] = (p.rgba[base + (fx >= 0.5f ? 1 : 0) + (fy >= 0.5f ? sy : 0) + (fz >= 0.5f ? sz : 0)] & 0x00ffffffu) | 0xff000000u;
            return;
        }
        prev = true;
        tp = ti;
    }
    render_miss(p, px);
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

size_t sde_tsdf_mesh_ws_bytes(int nx, int ny, int nz) {
    if (!dims_ok(nx, ny, nz)) return 0;
    const size_t total = (size_t)nx * ny * nz;
    return (2 * ((total + TILE - 1) / TILE) + total) * sizeof(unsigned);                 // vertex counts, quad counts, the cell -> vertex map
}

int sde_tsdf_mesh(const float* tsdf, const float* weight, const uint8_t* rgba, int nx, int ny, int nz, const float* origin, float voxel,
                  float min_weight, void* workspace, size_t workspace_bytes, void* vertices, long cap_vertices, int* faces, long cap_faces,
                  int* count, sde_stream_t stream) {
    SDE_CHECK_ARG(dims_ok(nx, ny, nz), "sde_tsdf_mesh: every dimension must lie in [1, %d] and their product be at most 2^30 (%d x %d x %d)", MAX_DIM, nx, ny,
                  nz);
    SDE_CHECK_ARG(voxel > 0.f, "sde_tsdf_mesh: voxel must be positive (%g)", (double)voxel);
    SDE_CHECK_ARG(min_weight >= 1.f, "sde_tsdf_mesh: min_weight must be at least 1 (%g)", (double)min_weight);
    SDE_CHECK_ARG(cap_vertices >= 1 && cap_vertices <= 0x7fffffffL && cap_faces >= 1 && cap_faces <= 0x7fffffffL,
                  "sde_tsdf_mesh: both caps must lie in [1, 2^31) (%ld, %ld)", cap_vertices, cap_faces);
    SDE_CHECK_ARG(tsdf && weight && origin && vertices && faces && count, "sde_tsdf_mesh: null pointer");
    SDE_CHECK_ARG(((uintptr_t)vertices & 15) == 0, "sde_tsdf_mesh: vertices must be 16-byte aligned");
    SDE_CHECK_ARG(((uintptr_t)faces & 3) == 0 && ((uintptr_t)rgba & 3) == 0, "sde_tsdf_mesh: faces and rgba must be 4-byte aligned");
    const size_t need = sde_tsdf_mesh_ws_bytes(nx, ny, nz);
    SDE_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
                  "sde_tsdf_mesh: workspace of %zu bytes, sde_tsdf_mesh_ws_bytes asks for %zu (4-byte aligned)", workspace ? workspace_bytes : (size_t)0, need);
    const size_t total = (size_t)nx * ny * nz, ntiles = (total + TILE - 1) / TILE;
    unsigned* ws = (unsigned*)workspace;
    MeshP p{PointsP{tsdf, weight, (const uint32_t*)rgba, ws, count, (uint4*)vertices, Grid{nx, ny, nz, origin[0], origin[1], origin[2], voxel}, total, ntiles,
                    (unsigned)cap_vertices, min_weight},
            ws + ntiles, ws + 2 * ntiles, faces, (size_t)cap_faces};
    const unsigned grid = (unsigned)(ntiles < (size_t)MAX_BLOCKS ? ntiles : (size_t)MAX_BLOCKS);
    hipLaunchKernelGGL(mesh_count, dim3(grid), dim3(TILE), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(mesh_scan, dim3(1), dim3(TILE), 0, (hipStream_t)stream, p.pt.ws, p.ws_q, count, ntiles);
    hipLaunchKernelGGL(mesh_vertices, dim3(grid), dim3(TILE), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(mesh_faces, dim3(grid), dim3(TILE), 0, (hipStream_t)stream, p);
    SDE_CHECK_LAUNCH("sde_tsdf_mesh");
    return SDE_OK;
}

int sde_tsdf_render(const float* tsdf, const float* weight, const uint8_t* rgba, int nx, int ny, int nz, const float* origin, float voxel,
                    float min_weight, const float* K, const float* C, int H, int W, float near, float step, int n, float* depth, float* normal,
                    uint8_t* picture, sde_stream_t stream) {
    SDE_CHECK_ARG(dims_ok(nx, ny, nz), "sde_tsdf_render: every dimension must lie in [1, %d] and their product be at most 2^30 (%d x %d x %d)", MAX_DIM, nx, ny,
                  nz);
    SDE_CHECK_ARG(voxel > 0.f, "sde_tsdf_render: voxel must be positive (%g)", (double)voxel);
    SDE_CHECK_ARG(min_weight >= 1.f, "sde_tsdf_render: min_weight must be at least 1 (%g)", (double)min_weight);
    SDE_CHECK_ARG(H >= 1 && W >= 1 && H <= MAX_PICTURE && W <= MAX_PICTURE, "sde_tsdf_render: H and W must lie in [1, %d] (%d x %d)", MAX_PICTURE, H, W);
    SDE_CHECK_ARG(n >= 1 && n <= MAX_SAMPLES, "sde_tsdf_render: the sample count must lie in [1, %d] (%d)", MAX_SAMPLES, n);
    SDE_CHECK_ARG(step > 0.f && step < INFINITY && fabsf(near) < INFINITY, "sde_tsdf_render: near must be finite, step positive and finite (%g, %g)",
                  (double)near, (double)step);                                                           // a NaN fails the comparison
    SDE_CHECK_ARG(tsdf && weight && origin && K && C && depth, "sde_tsdf_render: null pointer");
    SDE_CHECK_ARG(!picture || rgba, "sde_tsdf_render: a picture needs a volume with rgba");
    SDE_CHECK_ARG(((uintptr_t)rgba & 3) == 0 && ((uintptr_t)picture & 3) == 0, "sde_tsdf_render: rgba and picture must be 4-byte aligned");
    RenderP p{tsdf, weight, (const uint32_t*)rgba, K, C, depth, normal, (uint32_t*)picture, Grid{nx, ny, nz, origin[0], origin[1], origin[2], voxel},
              H, W, n, near, step, min_weight};
    const dim3 grid((unsigned)((W + RENDER_TW - 1) / RENDER_TW), (unsigned)((H + RENDER_TH - 1) / RENDER_TH));
    hipLaunchKernelGGL(tsdf_render, grid, dim3(RENDER_TW * RENDER_TH), 0, (hipStream_t)stream, p);
    SDE_CHECK_LAUNCH("sde_tsdf_render");
    return SDE_OK;
}

}  // extern "C"
