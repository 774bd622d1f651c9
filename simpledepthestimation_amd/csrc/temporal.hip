// Temporal fusion of depth over a frame sequence: the previous frame's (fused) depth is forward-projected into the current camera with the
// pose the model itself estimated, overlaps are resolved by a z-buffer, one-pixel holes are closed from the ring around them, and the result
// is blended with the current prediction where the two agree.  The contract is written out in include/sde_hip.h.
//
// sde_depth_warp_fuse, three launches ordered on the stream, one grid-stride grid each for all N maps:
//   zbuf_fill      every element of the z-buffer <- the bit pattern of +inf (zbuf.h);
//   warp_scatter   one pixel of the PREVIOUS frame per thread: lifted through the intrinsics, moved by [R | t + m], projected again, rounded
//                  to the nearest pixel (pinhole.h), then the z-buffer's minimum of the new depth (zbuf.h);
//   warp_fuse      one pixel of the CURRENT frame per thread: the z-buffer's entry, or -- where nothing landed -- the nearest entry of the up to
//                  eight neighbours; the consistency test, the blend, the class.
// Per pixel: 4 B of depth (+ 12 B of motion) read and one 4-byte atomic in the scatter; 4 B written by the fill; 4 B of z-buffer and 4 B of the
// current prediction read, 4 B + 1 B (+ 4 B) written by the fuse pass.  At the network's sizes (192 x 640: 0.5 MB per map) every launch is
// bound by launch and memory latency, not by bandwidth.
//
// `fused` may alias `prev` (read by the scatter alone, which has finished before the fuse pass starts) and `cur` (the fuse pass reads cur[i]
// and writes fused[i] in the same thread, and no other element of either): neither pointer carries __restrict__.
//
// Built with -ffp-contract=off: the projection and the blend keep the operation order the header states, which hip/temporal.py's host twin
// repeats bit for bit.
#include "common.h"
#include "pinhole.h"
#include "sde_hip.h"
#include "zbuf.h"

namespace {

constexpr int TILE = 256;
constexpr int MAX_BLOCKS = 2048;                 // 8 workgroups per compute unit; the grid-stride loops take the rest

struct WarpP {
    const float* prev;           // [N][h][w]
    const float* cur;            // [N][h][w]
    const float* K;              // [N][3][3]
    const float* T;              // [N][4][4]
    const float* motion;         // [N][3][h][w] or null
    unsigned* zbuf;              // [N][h][w]
    float* fused;                // [N][h][w]
    uint8_t* state;              // [N][h][w] or null
    float* warped;               // [N][h][w] or null
    int N, h, w;
    float alpha, tol;
};

__global__ void __launch_bounds__(TILE) warp_scatter(WarpP p) {
    const size_t plane = (size_t)p.h * p.w, total = (size_t)p.N * plane;
    for (size_t i = (size_t)blockIdx.x * TILE + threadIdx.x; i < total; i += (size_t)gridDim.x * TILE) {
        const int n = (int)(i / plane);
        const size_t at = i - (size_t)n * plane;
        const int v = (int)(at / p.w), u = (int)(at - (size_t)v * p.w);
        const float d = p.prev[i];
        const Pinhole c = pinhole_load(p.K + (size_t)n * 9);
        const float* T = p.T + (size_t)n * 16;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f;
        if (p.motion) {
            const float* mo = p.motion + (size_t)n * 3 * plane + at;
            m0 = mo[0]; m1 = mo[plane]; m2 = mo[2 * plane];
        }
        float px, py, qx, qy, qz, X, Y;
        pinhole_lift(c, (float)u, (float)v, d, px, py);
        pinhole_move<4>(T, px, py, d, T[3] + m0, T[7] + m1, T[11] + m2, qx, qy, qz);
        pinhole_project(c, qx, qy, qz, X, Y);
        const bool keep = fabsf(d) < INFINITY && d > 0.f && qz > 0.f && qz < INFINITY && fabsf(X) < INFINITY && fabsf(Y) < INFINITY;   // a NaN fails a comparison
        int ix, iy;
        if (!keep || !nearest_pixel(X, Y, ix, iy)) continue;
        if (ix < 0 || ix >= p.w || iy < 0 || iy >= p.h) continue;
        zbuf_min(p.zbuf + (size_t)n * plane + (size_t)iy * p.w + (size_t)ix, qz);
    }
}

__global__ void __launch_bounds__(TILE) warp_fuse(WarpP p) {
    const size_t plane = (size_t)p.h * p.w, total = (size_t)p.N * plane;
    for (size_t i = (size_t)blockIdx.x * TILE + threadIdx.x; i < total; i += (size_t)gridDim.x * TILE) {
        const size_t at = i % plane;
        const int y = (int)(at / p.w), x = (int)(at - (size_t)y * p.w);
        unsigned z = p.zbuf[i];
        bool filled = false;
        if (z == ZBUF_EMPTY) {                                                           // nothing landed here: the nearest of the ring around it
            const unsigned* zn = p.zbuf + (i - at);
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= p.h) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= p.w || (dx == 0 && dy == 0)) continue;
                    z = min(z, zn[(size_t)yy * p.w + xx]);                          // ZBUF_EMPTY is above every entry: it never wins
                }
            }
            filled = z != ZBUF_EMPTY;
        }
        const bool hole = z == ZBUF_EMPTY;
        const float wv = hole ? 0.f : __uint_as_float(z);
        const float c = p.cur[i];
        const bool c_ok = fabsf(c) < INFINITY && c > 0.f;
        const float diff = wv - c;
        const float lim = p.tol * fminf(wv, c);
        const bool usable = !hole && c_ok;
        const bool consistent = usable && fabsf(diff) <= lim;
        const float step = p.alpha * diff;
        p.fused[i] = consistent ? c + step : c;
        if (p.state) {
            const unsigned cls = !usable ? 0u : (consistent ? 1u : (diff < 0.f ? 2u : (diff > 0.f ? 3u : 0u)));
            p.state[i] = (uint8_t)(cls | (filled ? 4u : 0u));
        }
        if (p.warped) p.warped[i] = wv;
    }
}

unsigned blocks_for(size_t n) { return zbuf_blocks(n, TILE, MAX_BLOCKS); }

}  // namespace

extern "C" int sde_depth_warp_fuse(const float* prev, const float* cur, const float* K, const float* T, const float* motion, int N, int h, int w,
                                   float alpha, float tol, uint32_t* zbuf, float* fused, uint8_t* state, float* warped, sde_stream_t stream) {
    SDE_CHECK_ARG(N > 0 && h > 0 && w > 0, "sde_depth_warp_fuse: bad shape (N=%d, %dx%d)", N, h, w);
    SDE_CHECK_ARG(alpha >= 0.f && alpha < 1.f, "sde_depth_warp_fuse: alpha must lie in [0, 1) (%g)", (double)alpha);      // a NaN fails both
    SDE_CHECK_ARG(tol > 0.f, "sde_depth_warp_fuse: tol must be positive (%g)", (double)tol);
    SDE_CHECK_ARG(prev && cur && K && T && zbuf && fused, "sde_depth_warp_fuse: null pointer");
    SDE_CHECK_ARG((long)h * w <= 0x7fffffffL, "sde_depth_warp_fuse: map too large (%dx%d)", h, w);
    const size_t npx = (size_t)N * h * w;
    WarpP p{prev, cur, K, T, motion, (unsigned*)zbuf, fused, state, warped, N, h, w, alpha, tol};
    hipLaunchKernelGGL(zbuf_fill<TILE>, dim3(blocks_for(npx)), dim3(TILE), 0, (hipStream_t)stream, p.zbuf, npx);
    hipLaunchKernelGGL(warp_scatter, dim3(blocks_for(npx)), dim3(TILE), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(warp_fuse, dim3(blocks_for(npx)), dim3(TILE), 0, (hipStream_t)stream, p);
    SDE_CHECK_LAUNCH("sde_depth_warp_fuse");
    return SDE_OK;
}
