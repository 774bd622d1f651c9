// Projection of raw LiDAR scans to sparse depth maps: the inverse of cloud.hip.  The published routine is generate_depth_map of monodepth2 /
// packnet-sfm (project every scanner point with P_rect * R_rect * Tr_velo_to_cam, round, subtract the 1-based offset, keep the closest point per
// pixel); the contract, with its one deviation, is stated in include/sde_hip.h.
//
// sde_lidar_depth, three launches ordered on the stream, one grid-stride grid each for all B scans:
//   zbuf_fill       every element of the output window <- the bit pattern of +inf (zbuf.h);
//   lidar_scatter   one point per thread: three dot products, two divisions, the nearest pixel (pinhole.h), then the z-buffer's minimum (zbuf.h);
//   lidar_finish    +inf -> 0 (no point), everything else min(d, max_depth).
// Per frame at 120 k points and 375 x 1242: 1.4-1.9 MB of points read once, one 4-byte atomic per point that lands in the window, 1.9 MB of map
// written twice and read once.
//
// Built with -ffp-contract=off: u, v, w keep the operation order the header states, which hip/lidar.py's host twin repeats bit for bit.
#include "common.h"
#include "pinhole.h"
#include "sde_hip.h"
#include "zbuf.h"

namespace {

constexpr int TILE = 256;
constexpr int MAX_BLOCKS = 2048;                 // 8 workgroups per compute unit; the grid-stride loops take the rest

struct LidarP {
    const float* pts;            // [B][cap][stride]
    const int* count;            // [B]
    const float* proj;           // [B][3][4]
    const int* origin;           // [B][2]
    unsigned* depth;             // [B][H][W]
    int cap, stride, B, H, W, flags;
    float max_depth;
};

__global__ void __launch_bounds__(TILE) lidar_scatter(LidarP p) {
    const size_t total = (size_t)p.B * p.cap;
    for (size_t i = (size_t)blockIdx.x * TILE + threadIdx.x; i < total; i += (size_t)gridDim.x * TILE) {
        const int b = (int)(i / p.cap), k = (int)(i - (size_t)b * p.cap);
        if (k >= min(p.count[b], p.cap)) continue;                           // rows behind count[b] are never read; a count above cap cannot reach past the scan
        const float* q = p.pts + i * p.stride;
        const float x = q[0], y = q[1], z = q[2];
        const float* m = p.proj + (size_t)b * 12;
        const float u = m[0] * x + m[1] * y + m[2] * z + m[3];
        const float v = m[4] * x + m[5] * y + m[6] * z + m[7];
        const float w = m[8] * x + m[9] * y + m[10] * z + m[11];
        const float d = (p.flags & SDE_LIDAR_VEL_DEPTH) ? x : w;
        bool keep = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY && w > 0.f;      // NaN fails every comparison
        keep = keep && d > 0.f && d < INFINITY;
        if ((p.flags & SDE_LIDAR_FRONT_ONLY) && !(x >= 0.f)) keep = false;
        int iu, iv;
        if (!keep || !nearest_pixel(u / w, v / w, iu, iv)) continue;
        const long px = (long)iu - 1 - p.origin[2 * b], py = (long)iv - 1 - p.origin[2 * b + 1];
        if (px < 0 || px >= p.W || py < 0 || py >= p.H) continue;
        zbuf_min(p.depth + ((size_t)b * p.H + (size_t)py) * p.W + (size_t)px, d);
    }
}

__global__ void __launch_bounds__(TILE) lidar_finish(unsigned* __restrict__ depth, size_t n, float max_depth) {
    for (size_t i = (size_t)blockIdx.x * TILE + threadIdx.x; i < n; i += (size_t)gridDim.x * TILE) {
        const unsigned bits = depth[i];
        float d = bits == ZBUF_EMPTY ? 0.f : __uint_as_float(bits);
        if (max_depth > 0.f) d = fminf(d, max_depth);
        depth[i] = __float_as_uint(d);
    }
}

unsigned blocks_for(size_t n) { return zbuf_blocks(n, TILE, MAX_BLOCKS); }

}  // namespace

extern "C" int sde_lidar_depth(const float* pts, int cap, int stride, const int* count, int B, const float* proj, const int* origin, int H, int W,
                               int flags, float max_depth, float* depth, sde_stream_t stream) {
    SDE_CHECK_ARG(stride == 3 || stride == 4, "sde_lidar_depth: stride must be 3 or 4 (%d)", stride);
    SDE_CHECK_ARG(H > 0 && W > 0 && cap > 0 && B >= 0, "sde_lidar_depth: bad shape (B=%d, cap=%d, %dx%d)", B, cap, H, W);
    SDE_CHECK_ARG((flags & ~(SDE_LIDAR_VEL_DEPTH | SDE_LIDAR_FRONT_ONLY)) == 0, "sde_lidar_depth: unknown flag bits (%d)", flags);
    if (B == 0) return SDE_OK;
    SDE_CHECK_ARG(pts && count && proj && origin && depth, "sde_lidar_depth: null pointer");
    const size_t npx = (size_t)B * H * W;
    LidarP p{pts, count, proj, origin, (unsigned*)depth, cap, stride, B, H, W, flags, max_depth};
    hipLaunchKernelGGL(zbuf_fill<TILE>, dim3(blocks_for(npx)), dim3(TILE), 0, (hipStream_t)stream, p.depth, npx);
    hipLaunchKernelGGL(lidar_scatter, dim3(blocks_for((size_t)B * cap)), dim3(TILE), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(lidar_finish, dim3(blocks_for(npx)), dim3(TILE), 0, (hipStream_t)stream, p.depth, npx, max_depth);
    SDE_CHECK_LAUNCH("sde_lidar_depth");
    return SDE_OK;
}
