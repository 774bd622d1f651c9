// Optical flow A -> B from the depth of frame A and the relative pose (the reference's detectron2/geometry/camera.py: img_to_points L125-138 into
// points_to_img L141-163), as ONE launch per batch: sde_pair_flow.
//
// Every pixel (u, v) of the restored H x W map reads the network output -- and the per-pixel translation, when there is one -- through the index
// maps of sde_depth_present (-1 = outside: 0), is lifted through the source-size intrinsics, moved by [R | t + m], projected again, and goes out up
// to three times: as the flow (X - u, Y - v), as the validity byte, and as a colour of the 55-entry wheel under the camera frame.  The whole
// evaluation order is written out in include/sde_hip.h; the tests' bound counts its roundings, so this file is built with -ffp-contract=off.
//
// Streaming kernel with the gather pattern of present.hip, and walked the same way: a thread owns RUN consecutive pixels of the FLATTENED map, so
// each output of its run is one piece of memory written with the widest stores that divide it (RUN = 4: 32 B of flow as two dwordx4, 4 validity
// bytes as one dword, 12 B of colours as one dwordx3), rows end where they may and only the last run of an image can be short: that run takes the
// per-pixel path.  Per pixel: 4 B of depth gathered (+ 12 B of motion), 8 B + 1 B + 3 B written, 3 B in / 3 B out for the frame; K and T are
// the same for a whole workgroup.  The wheel sits in LDS as one packed dword per entry.  No atomics, no workspace, nothing read back: legal under
// graph capture, the same bytes every run.
#include "common.h"
#include "pinhole.h"
#include "sde_hip.h"
#include "wide_io.h"

namespace {

constexpr int RUN = 4;            // pixels per thread
constexpr int TPB = 256;          // threads per workgroup
constexpr int TILE = 1024;        // pixels per workgroup (the tests size their ragged case from this line)
constexpr int MAX_COLS = 256;     // wheel entries that fit the LDS table
static_assert(TILE == RUN * TPB && RUN % 4 == 0, "a run is a whole number of dwords in every output");

struct FlowP {
    const float* pred;           // [N][ph][pw]
    const int* ymap;             // [H]
    const int* xmap;             // [W]
    const float* K;              // [N][3][3]
    const float* T;              // [N][4][4]
    const float* motion;         // [N][3][ph][pw] or null
    const uint8_t* wheel;        // [ncols][3] or null (no canvas)
    const uint8_t* frame;        // [N][H][W][3] or null
    float* flow;                 // [N][H][W][2] or null
    uint8_t* valid;              // [N][H][W] or null
    uint8_t* canvas;             // [N][H or 2H][W][3] or null
    int H, W, ph, pw, ncols;
    float max_flow;
};

struct Cam {                     // what every pixel of one image shares besides the intrinsics
    float R[9], t[3], xlim, ylim;
};

__device__ __forceinline__ uint32_t channel(uint32_t w0, uint32_t w1, int shift, float f, float rad) {
    const float c0 = (float)((w0 >> shift) & 255u) / 255.f, c1 = (float)((w1 >> shift) & 255u) / 255.f;
    float col = (1.f - f) * c0 + f * c1;
    col = 1.f - rad * (1.f - col);
    const float v = 255.f * col;
    return v >= 255.f ? 255u : (v > 0.f ? (uint32_t)(int)v : 0u);
}

// the wheel colour of one flow vector (include/sde_hip.h states the definition), packed r | g << 8 | b << 16
__device__ __forceinline__ uint32_t flow_colour(float fx, float fy, float max_flow, const uint32_t* wheel, int ncols) {
    const float fu = fx / max_flow, fv = fy / max_flow;
    float rad = sqrtf(fu * fu + fv * fv);
    rad = rad < 1.f ? rad : 1.f;
    const float a = atan2f(-fv, -fu) / 3.14159265358979323846f;
    const float fk = (a + 1.f) * 0.5f * (float)(ncols - 1);
    int k0 = (int)fk;
    k0 = k0 < 0 ? 0 : (k0 > ncols - 1 ? ncols - 1 : k0);
    const int k1 = k0 + 1 == ncols ? 0 : k0 + 1;
    const float f = fk - (float)k0;
    const uint32_t w0 = wheel[k0], w1 = wheel[k1];
    return channel(w0, w1, 0, f, rad) | (channel(w0, w1, 8, f, rad) << 8) | (channel(w0, w1, 16, f, rad) << 16);
}

// one pixel: depth d and translation (m0, m1, m2) = t + m already formed -> flow and validity bits
__device__ __forceinline__ uint32_t project(const Pinhole& k, const Cam& c, bool inside, int u, int v, float d, float m0, float m1, float m2, float& fx,
                                            float& fy) {
    const float fu = (float)u, fv = (float)v;
    float px, py, qx, qy, qz, X, Y;
    pinhole_lift(k, fu, fv, d, px, py);
    pinhole_move<3>(c.R, px, py, d, m0, m1, m2, qx, qy, qz);
    pinhole_project(k, qx, qy, qz, X, Y);
    const bool b0 = inside && fabsf(d) < INFINITY && d > 0.f && qz > 0.f && fabsf(X) < INFINITY && fabsf(Y) < INFINITY;   // a NaN fails a comparison
    const bool b1 = b0 && X >= 0.f && X < c.xlim && Y >= 0.f && Y < c.ylim;
    fx = b0 ? X - fu : 0.f;
    fy = b0 ? Y - fv : 0.f;
    return (b0 ? 1u : 0u) | (b1 ? 2u : 0u);
}

__global__ void __launch_bounds__(TPB) pair_flow_kernel(FlowP p) {
    __shared__ uint32_t swheel[MAX_COLS];
    if (p.canvas) {                                                      // the same branch in every thread
        for (int i = threadIdx.x; i < p.ncols; i += TPB)
            swheel[i] = (uint32_t)p.wheel[3 * i] | ((uint32_t)p.wheel[3 * i + 1] << 8) | ((uint32_t)p.wheel[3 * i + 2] << 16);
        __syncthreads();
    }
    const int n = blockIdx.y, npx = p.H * p.W;
    const int p0 = (blockIdx.x * TPB + threadIdx.x) * RUN;
    if (p0 >= npx) return;
    const int cnt = min(RUN, npx - p0);
    const Pinhole k = pinhole_load(p.K + (size_t)n * 9);
    Cam c;
    {
        const float* T = p.T + (size_t)n * 16;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            c.R[3 * i] = T[4 * i]; c.R[3 * i + 1] = T[4 * i + 1]; c.R[3 * i + 2] = T[4 * i + 2];
            c.t[i] = T[4 * i + 3];
        }
        c.xlim = (float)(p.W - 1); c.ylim = (float)(p.H - 1);
    }
    const size_t plane = (size_t)p.ph * p.pw;
    const float* pr = p.pred + (size_t)n * plane;
    const float* mo = p.motion ? p.motion + (size_t)n * 3 * plane : nullptr;
    int y = p0 / p.W, x = p0 - y * p.W;
    int r = p.ymap[y];
    float fl[2 * RUN];
    uint32_t vb[RUN], col[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        fl[2 * j] = 0.f; fl[2 * j + 1] = 0.f; vb[j] = 0u; col[j] = 0u;
        if (j < cnt) {
            const int cc = p.xmap[x];
            const bool inside = r >= 0 && cc >= 0;
            float d = 0.f, m0 = 0.f, m1 = 0.f, m2 = 0.f;
            if (inside) {
                const size_t at = (size_t)r * p.pw + cc;
                d = pr[at];
                if (mo) { m0 = mo[at]; m1 = mo[plane + at]; m2 = mo[2 * plane + at]; }
            }
            vb[j] = project(k, c, inside, x, y, d, c.t[0] + m0, c.t[1] + m1, c.t[2] + m2, fl[2 * j], fl[2 * j + 1]);
            if (p.canvas && (vb[j] & 1u)) col[j] = flow_colour(fl[2 * j], fl[2 * j + 1], p.max_flow, swheel, p.ncols);
            if (++x == p.W) { x = 0; ++y; r = y < p.H ? p.ymap[y] : -1; }
        }
    }
    const size_t img = (size_t)n * npx;
    uint8_t* cv = p.canvas ? p.canvas + (p.frame ? 2 : 1) * img * 3 : nullptr;          // this image's canvas
    uint8_t* cc = cv ? cv + (p.frame ? (size_t)npx * 3 : 0) + (size_t)p0 * 3 : nullptr;   // ... and this run's colours in it
    const uint8_t* fr = (p.frame && cv) ? p.frame + (img + p0) * 3 : nullptr;
    if (cnt == RUN) {
        uint32_t w[2 * RUN];
        if (fr) {                                                       // the frame's bytes are on their way while the rest is packed
            get_dwords<3 * RUN / 4>(fr, w);
            put_dwords<3 * RUN / 4>(cv + (size_t)p0 * 3, w);
        }
        if (p.flow) {
#pragma unroll
            for (int j = 0; j < 2 * RUN; ++j) w[j] = __float_as_uint(fl[j]);
            put_dwords<2 * RUN>(p.flow + (img + p0) * 2, w);
        }
        if (p.valid) {
#pragma unroll
            for (int q = 0; q < RUN / 4; ++q) w[q] = vb[4 * q] | (vb[4 * q + 1] << 8) | (vb[4 * q + 2] << 16) | (vb[4 * q + 3] << 24);
            put_dwords<RUN / 4>(p.valid + img + p0, w);
        }
        if (cc) {
#pragma unroll
            for (int q = 0; q < RUN / 4; ++q) {                         // four 3-byte pixels fill three dwords
                const uint32_t a = col[4 * q], b = col[4 * q + 1], e = col[4 * q + 2], g = col[4 * q + 3];
                w[3 * q] = a | (b << 24);
                w[3 * q + 1] = (b >> 8) | (e << 16);
                w[3 * q + 2] = (e >> 16) | (g << 8);
            }
            put_dwords<3 * RUN / 4>(cc, w);
        }
        return;
    }
    // the image's last, short run: pixel by pixel
    for (int j = 0; j < RUN; ++j) {
        if (j >= cnt) break;
        if (p.flow) { p.flow[(img + p0 + j) * 2] = fl[2 * j]; p.flow[(img + p0 + j) * 2 + 1] = fl[2 * j + 1]; }
        if (p.valid) p.valid[img + p0 + j] = (uint8_t)vb[j];
        if (cc) { cc[3 * j] = (uint8_t)col[j]; cc[3 * j + 1] = (uint8_t)(col[j] >> 8); cc[3 * j + 2] = (uint8_t)(col[j] >> 16); }
        if (fr) {
            uint8_t* cf = cv + (size_t)(p0 + j) * 3;
            cf[0] = fr[3 * j]; cf[1] = fr[3 * j + 1]; cf[2] = fr[3 * j + 2];
        }
    }
}

}  // namespace

extern "C" {

int sde_pair_flow(const float* pred, int N, int ph, int pw, const int* ymap, const int* xmap, int H, int W, const float* K, const float* T,
                  const float* motion, const uint8_t* wheel, int ncols, float max_flow, const uint8_t* frame, float* flow, uint8_t* valid,
                  uint8_t* canvas, sde_stream_t stream) {
    SDE_CHECK_ARG(N > 0 && H > 0 && W > 0 && ph > 0 && pw > 0, "sde_pair_flow: bad shape (N=%d, %dx%d -> %dx%d)", N, ph, pw, H, W);
    SDE_CHECK_ARG(max_flow > 0.f, "sde_pair_flow: max_flow must be positive (%g)", (double)max_flow);
    SDE_CHECK_ARG(ncols > 0 && ncols <= MAX_COLS, "sde_pair_flow: ncols must lie in [1, %d] (%d)", MAX_COLS, ncols);
    SDE_CHECK_ARG(pred && ymap && xmap && K && T, "sde_pair_flow: null pointer");
    SDE_CHECK_ARG(flow || valid || canvas, "sde_pair_flow: no output asked for");
    SDE_CHECK_ARG(!canvas || wheel, "sde_pair_flow: a canvas needs the colour wheel");
    SDE_CHECK_ARG(N <= 65535 && (long)H * W <= 0x7fffffffL - TILE && (long)ph * pw <= 0x7fffffffL, "sde_pair_flow: batch or map too large");
    FlowP p{pred, ymap, xmap, K, T, motion, wheel, frame, flow, valid, canvas, H, W, ph, pw, ncols, max_flow};
    hipLaunchKernelGGL(pair_flow_kernel, dim3((unsigned)sde_cdiv((long)H * W, TILE), (unsigned)N), dim3(TPB), 0, (hipStream_t)stream, p);
    SDE_CHECK_LAUNCH("sde_pair_flow");
    return SDE_OK;
}

}  // extern "C"
