// Presentation of network outputs (the per-frame tail of the reference's tools/demo.py:L68-104) as ONE launch per batch: every pixel of the restored
// H x W map reads the network output through the index maps of the postprocess.backward() chain (the maps of sde_depth_metrics: -1 = outside,
// value 0) and goes out up to three times -- as the restored fp32 depth, as write_depth's uint16 (depth * 255, truncated) and as a colour of the
// 256-entry table at index min(255, (int)(d^gamma / vmax^gamma * 256)) (plt.imshow(depth ** 0.8, cmap, vmin=0, vmax=MAX_DEPTH ** 0.8), L77), under
// the camera frame when one is given (the stacked picture of L100-104).
//
// Streaming kernel: per pixel 4 B gathered (neighbouring pixels share cache lines, enlargements read less) + 4 B depth + 2 B uint16 + 3 B colour
// + 3 B in / 3 B out for the frame.  A thread owns RUN consecutive pixels of the FLATTENED map, so each output of its run is one piece of
// memory written with the widest stores that divide it (RUN = 4: 12 B of colours as one dwordx3, 16 B of depth as one dwordx4, 8 B of uint16 as
// one dwordx2; at RUN = 16 they would be three, four and two dwordx4).  The map is walked flat, across row ends, so W * 3 needs no alignment and only the last
// run of an image can be short: that one run takes the per-pixel path.  Canvas rows start at any byte (H * W * 3 is rarely a multiple of 16
// and callers pass views), so the wide accesses carry no alignment promise: the compiler still emits global_load / global_store_dwordx2..4 for
// them, which this target serves at any address.
// RUN trades store width against parallelism: a 375 x 1242 frame is 466 K pixels, i.e. 456 waves at RUN = 16 -- not two per compute unit -- and
// 1820 at RUN = 4.  The measurements behind the choice are in DESIGN.md section 21.
// The table sits in LDS as one packed dword per entry (1 KB).  No atomics, no workspace, nothing read back: legal under graph capture.
#include "common.h"
#include "sde_hip.h"
#include "wide_io.h"

namespace {

constexpr int RUN = 4;            // pixels per thread
constexpr int TPB = 256;          // threads per workgroup
static_assert(RUN % 4 == 0, "a run is a whole number of dwords in every output");

struct PresentP {
    const float* pred;           // [N][ph][pw]
    const int* ymap;             // [H]
    const int* xmap;             // [W]
    const uint8_t* lut;          // [256][3]
    const uint8_t* frame;        // [N][H][W][3] or null
    float* depth;                // [N][H][W] or null
    uint16_t* u16;               // [N][H][W] or null
    uint8_t* canvas;             // [N][H or 2H][W][3]
    int H, W, ph, pw;
    float vmax, gamma;
};

__device__ __forceinline__ int colour_index(float d, float gamma, float den) {
    if (!(d > 0.f)) return 0;                             // NaN, negative and zero
    const float s = powf(d, gamma) / den * 256.f;
    return s >= 255.f ? 255 : (int)s;                     // +inf lands here too
}
__device__ __forceinline__ uint32_t depth_u16(float d) {
    const float v = d * 255.f;                            // fp32 product, truncated: write_depth's (depth * 255).astype(uint16)
    return v >= 65535.f ? 65535u : (v > 0.f ? (uint32_t)(int)v : 0u);
}

__global__ void __launch_bounds__(TPB) present_kernel(PresentP p) {
    __shared__ uint32_t slut[256];
    for (int i = threadIdx.x; i < 256; i += TPB)
        slut[i] = (uint32_t)p.lut[3 * i] | ((uint32_t)p.lut[3 * i + 1] << 8) | ((uint32_t)p.lut[3 * i + 2] << 16);
    __syncthreads();
    const int n = blockIdx.y, npx = p.H * p.W;
    const int p0 = (blockIdx.x * TPB + threadIdx.x) * RUN;
    if (p0 >= npx) return;
    const int cnt = min(RUN, npx - p0);
    const float* pr = p.pred + (size_t)n * p.ph * p.pw;
    const float den = powf(p.vmax, p.gamma);
    int y = p0 / p.W, x = p0 - y * p.W;
    int r = p.ymap[y];
    float d[RUN];
    uint32_t col[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        d[j] = 0.f;
        if (j < cnt) {
            const int c = p.xmap[x];
            if (r >= 0 && c >= 0) d[j] = pr[(size_t)r * p.pw + c];
            if (++x == p.W) { x = 0; ++y; r = y < p.H ? p.ymap[y] : -1; }
        }
        col[j] = slut[colour_index(d[j], p.gamma, den)];
    }
    const size_t img = (size_t)n * npx;
    uint8_t* cv = p.canvas + (p.frame ? 2 : 1) * img * 3;               // this image's canvas
    uint8_t* cc = cv + (p.frame ? (size_t)npx * 3 : 0) + (size_t)p0 * 3;   // ... and this run's colours in it
    const uint8_t* fr = p.frame ? p.frame + (img + p0) * 3 : nullptr;
    if (cnt == RUN) {
        uint32_t w[RUN];
        if (fr) {                                                       // the frame's bytes are on their way while the rest is packed
            get_dwords<3 * RUN / 4>(fr, w);
            put_dwords<3 * RUN / 4>(cv + (size_t)p0 * 3, w);
        }
        if (p.depth) {
#pragma unroll
            for (int j = 0; j < RUN; ++j) w[j] = __float_as_uint(d[j]);
            put_dwords<RUN>(p.depth + img + p0, w);
        }
        if (p.u16) {
#pragma unroll
            for (int j = 0; j < RUN / 2; ++j) w[j] = depth_u16(d[2 * j]) | (depth_u16(d[2 * j + 1]) << 16);
            put_dwords<RUN / 2>(p.u16 + img + p0, w);
        }
#pragma unroll
        for (int q = 0; q < RUN / 4; ++q) {                             // four 3-byte pixels fill three dwords
            const uint32_t a = col[4 * q], b = col[4 * q + 1], c = col[4 * q + 2], e = col[4 * q + 3];
            w[3 * q] = a | (b << 24);
            w[3 * q + 1] = (b >> 8) | (c << 16);
            w[3 * q + 2] = (c >> 16) | (e << 8);
        }
        put_dwords<3 * RUN / 4>(cc, w);
        return;
    }
    // the image's last, short run: pixel by pixel
    for (int j = 0; j < RUN; ++j) {
        if (j >= cnt) break;
        if (p.depth) p.depth[img + p0 + j] = d[j];
        if (p.u16) p.u16[img + p0 + j] = (uint16_t)depth_u16(d[j]);
        cc[3 * j] = (uint8_t)col[j]; cc[3 * j + 1] = (uint8_t)(col[j] >> 8); cc[3 * j + 2] = (uint8_t)(col[j] >> 16);
        if (fr) {
            uint8_t* cf = cv + (size_t)(p0 + j) * 3;
            cf[0] = fr[3 * j]; cf[1] = fr[3 * j + 1]; cf[2] = fr[3 * j + 2];
        }
    }
}

}  // namespace

extern "C" {

int sde_depth_present(const float* pred, int N, int ph, int pw, const int* ymap, const int* xmap, int H, int W, float vmax, float gamma,
                      const uint8_t* lut, const uint8_t* frame, float* depth_full, uint16_t* depth_u16, uint8_t* canvas, sde_stream_t stream) {
    SDE_CHECK_ARG(N > 0 && H > 0 && W > 0 && ph > 0 && pw > 0, "sde_depth_present: bad shape (N=%d, %dx%d -> %dx%d)", N, ph, pw, H, W);
    SDE_CHECK_ARG(vmax > 0.f && gamma > 0.f, "sde_depth_present: vmax and gamma must be positive (%g, %g)", (double)vmax, (double)gamma);
    SDE_CHECK_ARG(pred && ymap && xmap && lut && canvas, "sde_depth_present: null pointer");
    SDE_CHECK_ARG(N <= 65535 && (long)H * W <= 0x7fffffffL - RUN * TPB && (long)ph * pw <= 0x7fffffffL, "sde_depth_present: batch or map too large");
    PresentP p{pred, ymap, xmap, lut, frame, depth_full, depth_u16, canvas, H, W, ph, pw, vmax, gamma};
    hipLaunchKernelGGL(present_kernel, dim3((unsigned)sde_cdiv((long)H * W, RUN * TPB), (unsigned)N), dim3(TPB), 0, (hipStream_t)stream, p);
    SDE_CHECK_LAUNCH("sde_depth_present");
    return SDE_OK;
}

}  // extern "C"
