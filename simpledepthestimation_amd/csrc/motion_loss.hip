// MotionLearning loss stack for gfx950 (MI355X): view synthesis with a per-pixel translation, the RGB-D consistency loss (warp + 4-channel
// gather + per-sample reductions + weighted SSIM), the stand-alone WeightedSSIM, the motion consistency / smoothness / sparsity terms and the
// adaptive average pool of the image pyramid.
//
// Replaces (reference, read-only): detectron2/geometry/camera.py:L49-54,L166-202 with t [B,3,H,W], detectron2/modeling/losses/ssim_loss.py:L56-111,
// detectron2/modeling/losses/motion_loss.py:L7-64 and detectron2/modeling/meta_arch/MotionLearning.py:L248-291.
//
// Numerics: fp32, planar NCHW.  Compiled with -ffp-contract=off like photometric.hip: the projection keeps that file's operation order (projection.h),
// the only difference being K @ t evaluated per pixel.  One workgroup = 4 rows of 64 pixels of one sample (a wave reads one contiguous 256 B row
// segment per plane); the 3x3 neighbourhoods of the SSIM kernels are re-read through L1 / L2.  Per-sample camera values live in scalar registers.
// Reductions: per-workgroup partials in a fixed order, then a finalize; the only float atomics are the bilinear scatter of mc_bwd_kernel.
#include "common.h"
#include "projection.h"
#include "sde_hip.h"

namespace {

constexpr int PB_N = 256;     // 64 x 4 pixels per workgroup

// K, K^-1 and K @ R of one sample (make_cam with unit scale factors and a 3x3 rotation); kt is set per pixel
__device__ __forceinline__ void make_cam_rt(const float* __restrict__ K, const float* __restrict__ R, Cam& c) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { c.k[i] = K[i]; c.ki[i] = K[i]; }
    c.ki[0] = 1.0f / c.k[0];
    c.ki[4] = 1.0f / c.k[4];
    c.ki[2] = (-1.0f * c.k[2]) / c.k[0];
    c.ki[5] = (-1.0f * c.k[5]) / c.k[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.kr[3 * i + j] = (c.k[3 * i] * R[j] + c.k[3 * i + 1] * R[3 + j]) + c.k[3 * i + 2] * R[6 + j];
        c.kt[i] = 0.f;
    }
    c = cam_uniform(c);
}

// K @ t of this pixel: the chain of make_cam's kt
__device__ __forceinline__ void set_kt(Cam& c, float t0, float t1, float t2) {
#pragma unroll
    for (int i = 0; i < 3; ++i) c.kt[i] = fmaf(c.k[3 * i + 2], t2, fmaf(c.k[3 * i + 1], t1, c.k[3 * i] * t0));
}

__device__ __forceinline__ bool proj_valid(const Proj& pr, int W, int H) {
    const bool fin = (pr.X == pr.X) && fabsf(pr.X) <= kFltMax && (pr.Y == pr.Y) && fabsf(pr.Y) <= kFltMax;
    return fin && pr.X >= 0.f && pr.X < (float)(W - 1) && pr.Y >= 0.f && pr.Y < (float)(H - 1) && pr.q[2] > 0.f;
}

__device__ __forceinline__ void store_grid(const Proj& pr, int W, int H, float* __restrict__ g) {
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const float xs = fminf(fmaxf(nan_to_num(pr.X), 0.f), wm1), ys = fminf(fmaxf(nan_to_num(pr.Y), 0.f), hm1);
    g[0] = (2.0f * xs) / wm1 - 1.0f;
    g[1] = (2.0f * ys) / hm1 - 1.0f;
}

// ------------------------------------------------------------------------------------------------
// view_synthesis with t [B,3,H,W] (camera.py:L166-202): the outputs of view_synthesis_kernel
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PB_N) view_synthesis_pp_kernel(const float* __restrict__ img, const float* __restrict__ depth, const float* __restrict__ K,
                                                                 const float* __restrict__ R, const float* __restrict__ t, int C, int H, int W,
                                                                 float* __restrict__ sampled, float* __restrict__ Zout, float* __restrict__ grid,
                                                                 uint8_t* __restrict__ valid) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    Cam cam;
    make_cam_rt(K + 9 * b, R + 9 * b, cam);
    const long pix = (long)y * W + x;
    const long hw = (long)H * W;
    const float* tp = t + (long)b * 3 * hw + pix;
    set_kt(cam, tp[0], tp[hw], tp[2 * hw]);
    Proj pr;
    project(cam, x, y, depth[b * hw + pix], W, H, pr);
    Taps tp4;
    make_taps(pr.ix, pr.iy, W, H, tp4);
    for (int c = 0; c < C; ++c) sampled[((long)b * C + c) * hw + pix] = bilinear(img + ((long)b * C + c) * hw, W, tp4, nullptr);
    if (Zout) Zout[b * hw + pix] = fmaxf(pr.q[2], 1e-5f);
    if (grid) store_grid(pr, W, H, grid + (b * hw + pix) * 2);
    if (valid) valid[b * hw + pix] = proj_valid(pr, W, H) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// RGB-D consistency (MotionLearning.py:L248-291), pass 1: warp, gather frame_B + depth_B, masks, per-workgroup partial sums
// ------------------------------------------------------------------------------------------------
struct RgbdArgs {
    const float *fA, *fB, *dA, *dB, *K, *R, *t;
    int N, H, W;
    float* sampled;   // [N,3,H,W] warped frame_B
    float* grid;      // [N,H,W,2]
    float* occ;       // [N,1,H,W] occlusion mask (0 / 1)
    float* err;       // [N,1,H,W] depth_in_B - sampled_depth_B (signed; the SSIM weight squares it, the backward takes its sign)
    uint8_t* valid;   // [N,1,H,W] projection mask
    float* partial;   // [workgroups][4]: sum occ, sum err^2 occ, sum |sampled - frame_A| occ, sum |err| occ
};

__global__ void __launch_bounds__(PB_N) rgbd_warp_kernel(const RgbdArgs a) {
    __shared__ float red[16];
    const int n = blockIdx.z, H = a.H, W = a.W;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool act = x < W && y < H;
    const long hw = (long)H * W, pix = act ? (long)y * W + x : 0;
    Cam cam;
    make_cam_rt(a.K + 9 * n, a.R + 9 * n, cam);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (act) {
        const float* tp = a.t + (long)n * 3 * hw + pix;
        set_kt(cam, tp[0], tp[hw], tp[2 * hw]);
        Proj pr;
        project(cam, x, y, a.dA[n * hw + pix], W, H, pr);
        Taps t4;
        make_taps(pr.ix, pr.iy, W, H, t4);
        const float Z = fmaxf(pr.q[2], 1e-5f);
        const float sD = bilinear(a.dB + n * hw, W, t4, nullptr);
        const bool ok = proj_valid(pr, W, H);
        const float occ = (Z < sD && ok) ? 1.f : 0.f;
        const float e = Z - sD;
        float l1 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long o = ((long)n * 3 + c) * hw;
            const float s = bilinear(a.fB + o, W, t4, nullptr);
            a.sampled[o + pix] = s;
            l1 += fabsf(s - a.fA[o + pix]) * occ;
        }
        store_grid(pr, W, H, a.grid + (n * hw + pix) * 2);
        a.occ[n * hw + pix] = occ;
        a.err[n * hw + pix] = e;
        a.valid[n * hw + pix] = ok ? 1 : 0;
        v[0] = occ; v[1] = (e * e) * occ; v[2] = l1; v[3] = fabsf(sD - Z) * occ;
    }
    const int blk = (n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    sde_block_sums<4, PB_N / 64>(v, red, a.partial + 4 * (long)blk);
}

// ------------------------------------------------------------------------------------------------
// WeightedSSIM (ssim_loss.py:L56-111).  mode 0: both factors, 1: C1 == inf (structure term only), 2: C2 == inf (luminance term only).
// The weight comes from a map (stand-alone operator, backward) or is formed on the fly from pass 1's depth error (RGB-D pass 2):
// w = m2 / (err^2 + m2) * valid with m2 = sum(err^2 occ) / (sum(occ) + 1) + 1e-4 of the sample.
// ------------------------------------------------------------------------------------------------
struct WssimArgs {
    const float *x, *y;
    const float* w;            // [N,1,H,W] or null
    const float* err;          // w == null: pass 1's outputs
    const uint8_t* valid;
    const float* part1;        // [N * bps][4]
    int N, C, H, W, mode;
    float C1, C2;
    float* map;                // [N,C,H,W] or null
    float* avg_w;              // [N,1,H,W] or null
    float* wout;               // [N,1,H,W] or null: the weight itself (depth_proximity_weight)
    float* partial;            // [workgroups] or null: sum over channels and pixels of map * avg_w
};

struct Win {
    int off[9];
    float wp[9];     // w + 1e-2 at the reflected taps
    float aw;        // avg_pool2d(w, 3, 1, padding=1): zeros outside, divided by 9
    float wc;        // w at the centre
};

__device__ __forceinline__ float wssim_weight(const WssimArgs& a, long idx, float m2) {
    if (a.w) return a.w[idx];
    const float e = a.err[idx];
    return (m2 / (e * e + m2)) * (a.valid[idx] ? 1.f : 0.f);
}

__device__ __forceinline__ void make_win(const WssimArgs& a, int n, int x, int y, float m2, Win& w) {
    const long hw = (long)a.H * a.W;
    float aw = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int ry = reflect_idx(y + dy, a.H);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int rx = reflect_idx(x + dx, a.W), k = (dy + 1) * 3 + dx + 1;
            w.off[k] = ry * a.W + rx;
            const float wv = wssim_weight(a, n * hw + w.off[k], m2);
            if (y + dy >= 0 && y + dy < a.H && x + dx >= 0 && x + dx < a.W) aw += wv;
            if (k == 4) w.wc = wv;
            w.wp[k] = wv + 1e-2f;
        }
    }
    w.aw = aw / 9.0f;
}

struct Mom { float mx, my, n1, n2, d1, d2, n, d, inv; };

__device__ __forceinline__ float wssim_value(const float* __restrict__ xs, const float* __restrict__ ys, const Win& w, int mode, float C1, float C2, Mom& m) {
    float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float xv = xs[w.off[k]], yv = ys[w.off[k]], wp = w.wp[k];
        sx += xv * wp; sy += yv * wp; sxx += (xv * xv) * wp; syy += (yv * yv) * wp; sxy += (xv * yv) * wp;
    }
    const float inv9 = 1.0f / 9.0f;
    m.inv = 1.0f / (w.aw + 1e-2f);
    m.mx = (sx * inv9) * m.inv; m.my = (sy * inv9) * m.inv;
    const float vx = (sxx * inv9) * m.inv - m.mx * m.mx, vy = (syy * inv9) * m.inv - m.my * m.my, vxy = (sxy * inv9) * m.inv - m.mx * m.my;
    m.n1 = mode == 1 ? 1.f : 2.0f * m.mx * m.my + C1;
    m.d1 = mode == 1 ? 1.f : m.mx * m.mx + m.my * m.my + C1;
    m.n2 = mode == 2 ? 1.f : 2.0f * vxy + C2;
    m.d2 = mode == 2 ? 1.f : vx + vy + C2;
    m.n = m.n1 * m.n2; m.d = m.d1 * m.d2;
    return (1.0f - m.n / m.d) * 0.5f;
}

// normalizer - 1 and the depth error's second moment of sample n from pass 1's partials: every workgroup of the sample adds them in the same order
__device__ __forceinline__ float sample_m2(const float* __restrict__ part1, int n, int bps, float* red) {
    __shared__ float tot[2], m2s;
    float v[2] = {0.f, 0.f};                                       // sum occ, sum err^2 occ: the first two of pass 1's four values
    sde_partial_walk<2, PB_N>(v, part1, (long)n * bps, bps, threadIdx.x, 4);
    sde_block_sums<2, PB_N / 64>(v, red, tot);
    __syncthreads();
    if (threadIdx.x == 0) m2s = tot[1] / (tot[0] + 1.0f) + 1e-4f;
    __syncthreads();
    return m2s;
}

__global__ void __launch_bounds__(PB_N) wssim_fwd_kernel(const WssimArgs a) {
    __shared__ float red[16];
    const int n = blockIdx.z, H = a.H, W = a.W;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool act = x < W && y < H;
    const long hw = (long)H * W, pix = act ? (long)y * W + x : 0;
    const float m2 = a.w ? 0.f : sample_m2(a.part1, n, gridDim.x * gridDim.y, red);
    float acc = 0.f;
    if (act) {
        Win w;
        make_win(a, n, x, y, m2, w);
        for (int c = 0; c < a.C; ++c) {
            const long o = ((long)n * a.C + c) * hw;
            Mom m;
            const float l = fminf(fmaxf(wssim_value(a.x + o, a.y + o, w, a.mode, a.C1, a.C2, m), 0.f), 1.f);
            if (a.map) a.map[o + pix] = l;
            acc += l * w.aw;
        }
        if (a.avg_w) a.avg_w[n * hw + pix] = w.aw;
        if (a.wout) a.wout[n * hw + pix] = w.wc;
    }
    if (a.partial) {
        const float s = sde_block_sum(acc, red);
        if (threadIdx.x == 0) a.partial[(n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
    }
}

// Backward, step 1: per window and channel the four coefficients of d(loss)/d(weighted window sums): (sum x wp, sum y wp, sum x^2 wp = sum y^2 wp, sum xy wp),
// the 1/9 of the pool folded in.  Upstream: gmap [N,C,H,W] (d loss / d map), or gvec[n] * gscale * avg_w (the RGB-D loss: mean of map * avg_w).
__global__ void __launch_bounds__(PB_N) wssim_coef_kernel(const WssimArgs a, const float* __restrict__ gmap, const float* __restrict__ gvec, float gscale,
                                                          float* __restrict__ coef) {
    const int n = blockIdx.z, H = a.H, W = a.W;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const long hw = (long)H * W, pix = (long)y * W + x;
    Win w;
    make_win(a, n, x, y, 0.f, w);
    for (int c = 0; c < a.C; ++c) {
        const long o = ((long)n * a.C + c) * hw;
        Mom m;
        const float l = wssim_value(a.x + o, a.y + o, w, a.mode, a.C1, a.C2, m);
        float4 k = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l >= 0.f && l <= 1.f) {                       // clamp passes the gradient on [0, 1] only
            const float g = gmap ? gmap[o + pix] : gvec[n] * gscale * w.aw;
            const float f = -0.5f * g * (1.0f / 9.0f);
            const float rd = 1.0f / m.d;
            const float an1 = a.mode == 1 ? 0.f : m.n2 * rd, an2 = a.mode == 2 ? 0.f : m.n1 * rd;
            const float ad1 = a.mode == 1 ? 0.f : -m.n * m.d2 * rd * rd, ad2 = a.mode == 2 ? 0.f : -m.n * m.d1 * rd * rd;
            // means enter n1 / d1 directly and the (co)variances through - mu^2, - mu_x mu_y
            const float dmx = (an1 * 2.0f * m.my + ad1 * 2.0f * m.mx) - 2.0f * m.mx * ad2 - m.my * 2.0f * an2;
            const float dmy = (an1 * 2.0f * m.mx + ad1 * 2.0f * m.my) - 2.0f * m.my * ad2 - m.mx * 2.0f * an2;
            k = make_float4(f * dmx * m.inv, f * dmy * m.inv, f * ad2 * m.inv, f * 2.0f * an2 * m.inv);
        }
        reinterpret_cast<float4*>(coef)[o + pix] = k;
    }
}

// sum over the (up to nine) windows that contain pixel (px, py) of the window coefficients applied to it, with the multiplicity reflection gives border taps
__device__ __forceinline__ void wssim_gather(const float* __restrict__ coef, long plane, int H, int W, int px, int py, float xv, float yv, float& gx, float& gy) {
    gx = 0.f; gy = 0.f;
#pragma unroll
    for (int ey = -1; ey <= 1; ++ey) {
        const int wy = py + ey;
        if (wy < 0 || wy >= H) continue;
        const float my_ = ((py == 1 && ey == -1) || (py == H - 2 && ey == 1)) ? 2.f : 1.f;
#pragma unroll
        for (int ex = -1; ex <= 1; ++ex) {
            const int wx = px + ex;
            if (wx < 0 || wx >= W) continue;
            const float mx_ = ((px == 1 && ex == -1) || (px == W - 2 && ex == 1)) ? 2.f : 1.f;
            const float4 c = reinterpret_cast<const float4*>(coef)[plane + (long)wy * W + wx];
            const float m = my_ * mx_;
            gx += m * (c.x + 2.0f * xv * c.z + yv * c.w);
            gy += m * (c.y + 2.0f * yv * c.z + xv * c.w);
        }
    }
}

__global__ void __launch_bounds__(PB_N) wssim_gather_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ w,
                                                            const float* __restrict__ coef, int C, int H, int W, float* __restrict__ dx, float* __restrict__ dy) {
    const int n = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const long hw = (long)H * W, pix = (long)y * W + x;
    const float wp = w[n * hw + pix] + 1e-2f;
    for (int c = 0; c < C; ++c) {
        const long o = ((long)n * C + c) * hw;
        float gx, gy;
        wssim_gather(coef, o, H, W, x, y, xs[o + pix], ys[o + pix], gx, gy);
        if (dx) dx[o + pix] = wp * gx;
        if (dy) dy[o + pix] = wp * gy;
    }
}

// per-sample results of the RGB-D forward: stats [4][N] = sum |sampled - frame_A| occ, sum map * avg_w, sum |err| occ / normalizer, normalizer
__global__ void __launch_bounds__(PB_N) rgbd_finalize_kernel(const float* __restrict__ part1, const float* __restrict__ part2, int bps, int N, float* __restrict__ stats) {
    __shared__ float red[20];
    const int n = blockIdx.x;
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    sde_partial_walk<4, PB_N>(v, part1, (long)n * bps, bps, threadIdx.x);
    if (part2) sde_partial_walk<1, PB_N>(v + 4, part2, (long)n * bps, bps, threadIdx.x);
    __shared__ float tot[5];
    sde_block_sums<5, PB_N / 64>(v, red, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        const float nrm = tot[0] + 1.0f;
        stats[n] = tot[2];
        stats[N + n] = tot[4];
        stats[2 * N + n] = tot[3] / nrm;
        stats[3 * N + n] = nrm;
    }
}

// RGB-D backward, step 2: SSIM gather + L1 terms -> d sampled -> bilinear sample -> projection: d depth_A, d t per pixel, d R per workgroup
struct RgbdBwdArgs {
    const float *fA, *fB, *dA, *K, *R, *t;
    const float *sampled, *occ, *err, *dpw, *coef /* null: no SSIM term */, *stats;
    const float *g_l1, *g_dl1;                   // [N] upstream gradients of stats rows 0 and 2 (null: zero)
    int N, H, W;
    float *d_depth, *d_t, *dR_partial;           // [N,1,H,W], [N,3,H,W], [workgroups][9]
};

__global__ void __launch_bounds__(PB_N) rgbd_bwd_kernel(const RgbdBwdArgs a) {
    __shared__ float red[36];
    const int n = blockIdx.z, H = a.H, W = a.W;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool act = x < W && y < H;
    const long hw = (long)H * W, pix = act ? (long)y * W + x : 0;
    Cam cam;
    make_cam_rt(a.K + 9 * n, a.R + 9 * n, cam);
    const float gl1 = a.g_l1 ? sde_uniform(a.g_l1[n]) : 0.f;
    const float gdl = a.g_dl1 ? sde_uniform(a.g_dl1[n]) / sde_uniform(a.stats[3 * a.N + n]) : 0.f;
    float acc9[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc9[i] = 0.f;
    if (act) {
        const float occ = a.occ[n * hw + pix];
        const float wp = a.coef ? a.dpw[n * hw + pix] + 1e-2f : 0.f;
        float ds[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long o = ((long)n * 3 + c) * hw;
            const float xv = a.sampled[o + pix], yv = a.fA[o + pix];
            float gx = 0.f, gy = 0.f;
            if (a.coef) wssim_gather(a.coef, o, H, W, x, y, xv, yv, gx, gy);
            const float df = xv - yv;
            const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
            ds[c] = wp * gx + gl1 * occ * sg;
        }
        const float* tp = a.t + (long)n * 3 * hw + pix;
        set_kt(cam, tp[0], tp[hw], tp[2 * hw]);
        Proj pr;
        project(cam, x, y, a.dA[n * hw + pix], W, H, pr);
        Taps t4;
        make_taps(pr.ix, pr.iy, W, H, t4);
        float dix = 0.f, diy = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v4[4];
            bilinear(a.fB + ((long)n * 3 + c) * hw, W, t4, v4);
            dix += ds[c] * ((v4[1] - v4[0]) * t4.sy + (v4[3] - v4[2]) * t4.ny);
            diy += ds[c] * ((v4[2] - v4[0]) * t4.ex + (v4[3] - v4[1]) * t4.wx);
        }
        const float dX = pr.passx ? dix : 0.f, dY = pr.passy ? diy : 0.f;
        // depth L1: |sampled_depth_B.detach() - Z| occ / normalizer; Z = clamp(q2, min=1e-5) passes the gradient where q2 >= 1e-5
        const float e = a.err[n * hw + pix];
        const float dZ = (occ != 0.f && pr.q[2] >= 1e-5f) ? gdl * (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) : 0.f;
        const float rden = 1.0f / (pr.q[2] + kEps);
        float dq[3];
        dq[0] = dX * rden; dq[1] = dY * rden;
        dq[2] = -(dX * pr.X + dY * pr.Y) * rden + dZ;
        const float fxp = (float)x, fyp = (float)y;
        float dd = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float dp = dq[0] * cam.kr[k] + dq[1] * cam.kr[3 + k] + dq[2] * cam.kr[6 + k];
            dd += dp * (cam.ki[3 * k] * fxp + cam.ki[3 * k + 1] * fyp + cam.ki[3 * k + 2]);
        }
        a.d_depth[n * hw + pix] = dd;
        // q = (K R) p + K t  ->  d t_m = sum_i K_im dq_i ; d R_mk = (sum_i K_im dq_i) p_k
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const float kq = cam.k[m] * dq[0] + cam.k[3 + m] * dq[1] + cam.k[6 + m] * dq[2];
            a.d_t[((long)n * 3 + m) * hw + pix] = kq;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc9[3 * m + k] = kq * pr.p[k];
        }
    }
    const int blk = (n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    sde_block_sums<9, PB_N / 64>(acc9, red, a.dR_partial + 9 * (long)blk);
}

// the nine sums of sample n over its bps per-workgroup partials, in every lane: one wave per sample, lanes split the partials, fixed butterfly
__device__ __forceinline__ void sample_sum9(const float* __restrict__ partial, int n, int bps, float (&acc)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.f;
    sde_partial_walk<9, 64>(acc, partial, (long)n * bps, bps, threadIdx.x);
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = sde_wave_sum(acc[i]);
}

// d R [N,3,3] from the per-workgroup partials
__global__ void __launch_bounds__(64) sum9_finalize_kernel(const float* __restrict__ partial, int bps, float* __restrict__ dR) {
    const int n = blockIdx.x, lane = threadIdx.x;
    float acc[9];
    sample_sum9(partial, n, bps, acc);
    if (lane < 9) dR[n * 9 + lane] = sde_lane_pick(acc, lane);
}

// ------------------------------------------------------------------------------------------------
// motion_consistency_loss (motion_loss.py:L7-48)
// ------------------------------------------------------------------------------------------------
struct McPix { float s[3], e[3], tA[3], E, den; Taps t4; };

__device__ __forceinline__ void mc_pixel(const float* __restrict__ grid, const float* __restrict__ R, const float* __restrict__ tA, const float* __restrict__ tB,
                                         int n, long pix, int H, int W, McPix& o) {
    const long hw = (long)H * W;
    const float gx = grid[(n * hw + pix) * 2], gy = grid[(n * hw + pix) * 2 + 1];
    const float ix = (gx + 1.0f) * ((float)(W - 1) / 2.0f), iy = (gy + 1.0f) * ((float)(H - 1) / 2.0f);      // grid_sample, align_corners=True
    make_taps(ix, iy, W, H, o.t4);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o.s[c] = bilinear(tB + ((long)n * 3 + c) * hw, W, o.t4, nullptr);
        o.tA[c] = tA[((long)n * 3 + c) * hw + pix];
        s1 += o.tA[c] * o.tA[c]; s2 += o.s[c] * o.s[c];
    }
    o.E = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o.e[i] = (R[3 * i] * o.s[0] + R[3 * i + 1] * o.s[1] + R[3 * i + 2] * o.s[2]) + o.tA[i];
        o.E += o.e[i] * o.e[i];
    }
    o.den = s1 + s2 + 1e-24f;
}

__global__ void __launch_bounds__(PB_N) mc_fwd_kernel(const float* __restrict__ grid, const float* __restrict__ mask, const float* __restrict__ R1,
                                                      const float* __restrict__ tA, const float* __restrict__ tB, int H, int W, float* __restrict__ partial) {
    __shared__ float red[16];
    const int n = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    float v = 0.f;
    if (x < W && y < H) {
        const long pix = (long)y * W + x;
        float R[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = sde_uniform(R1[n * 9 + i]);
        McPix p;
        mc_pixel(grid, R, tA, tB, n, pix, H, W, p);
        v = mask[(long)n * H * W + pix] * (p.E / p.den);
    }
    const float s = sde_block_sum(v, red);
    if (threadIdx.x == 0) partial[(n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
}

// v / den^2.  By den * den wherever that square is a normal fp32 number (the operation order every recorded result has); by den twice where it is not:
// with both rotations the identity, or both translations zero, den is the 1e-24f guard alone, its square is 0 in fp32 and v / (den * den) was 0 / 0.
__device__ __forceinline__ float div_sq(float v, float den) {
    const float d2 = den * den;
    return d2 >= 1.17549435e-38f ? v / d2 : v / den / den;
}

// rotation part of one sample: r = mean((R1 R2 - I)^2) / (mean((R1 - I)^2) + mean((R2 - I)^2) + 1e-24); optionally its gradient * g
__device__ __forceinline__ float mc_rot(const float* __restrict__ R1, const float* __restrict__ R2, float g, float* dR1, float* dR2) {
    float M[9], A[9], B[9], re = 0.f, a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float id = i == j ? 1.f : 0.f;
            M[3 * i + j] = ((R1[3 * i] * R2[j] + R1[3 * i + 1] * R2[3 + j]) + R1[3 * i + 2] * R2[6 + j]) - id;
            A[3 * i + j] = R1[3 * i + j] - id; B[3 * i + j] = R2[3 * i + j] - id;
            re += M[3 * i + j] * M[3 * i + j]; a += A[3 * i + j] * A[3 * i + j]; b += B[3 * i + j] * B[3 * i + j];
        }
    re = re / 9.0f; a = a / 9.0f; b = b / 9.0f;
    const float den = a + b + 1e-24f;
    if (dR1) {
        const float gm = g / den * (2.0f / 9.0f), gs = div_sq(-g * re, den) * (2.0f / 9.0f);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                // d R1 = dM R2^T, d R2 = R1^T dM
                dR1[3 * i + j] = gm * (M[3 * i] * R2[3 * j] + M[3 * i + 1] * R2[3 * j + 1] + M[3 * i + 2] * R2[3 * j + 2]) + gs * A[3 * i + j];
                dR2[3 * i + j] = gm * (R1[i] * M[j] + R1[3 + i] * M[3 + j] + R1[6 + i] * M[6 + j]) + gs * B[3 * i + j];
            }
    }
    return re / den;
}

// out[0] = rot_error, out[1] = trans_error (one workgroup)
__global__ void __launch_bounds__(PB_N) mc_finalize_kernel(const float* __restrict__ partial, int nblk, const float* __restrict__ R1, const float* __restrict__ R2,
                                                           int N, float inv_pixels, float* __restrict__ out) {
    __shared__ float red[16];
    float s = 0.f, r = 0.f;
    for (int i = threadIdx.x; i < nblk; i += PB_N) s += partial[i];
    for (int n = threadIdx.x; n < N; n += PB_N) r += mc_rot(R1 + 9 * n, R2 + 9 * n, 0.f, nullptr, nullptr);
    s = sde_block_sum(s, red);
    r = sde_block_sum(r, red);
    if (threadIdx.x == 0) { out[0] = r / (float)N; out[1] = s * inv_pixels; }
}

__global__ void __launch_bounds__(PB_N) mc_bwd_kernel(const float* __restrict__ grid, const float* __restrict__ mask, const float* __restrict__ R1,
                                                      const float* __restrict__ tA, const float* __restrict__ tB, const float* __restrict__ g_trans, float inv_pixels,
                                                      int H, int W, float* __restrict__ d_tA, float* __restrict__ d_tB, float* __restrict__ dR_partial) {
    __shared__ float red[36];
    const int n = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const long hw = (long)H * W;
    float acc9[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc9[i] = 0.f;
    if (x < W && y < H) {
        const long pix = (long)y * W + x;
        float R[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = sde_uniform(R1[n * 9 + i]);
        McPix p;
        mc_pixel(grid, R, tA, tB, n, pix, H, W, p);
        const float g = (g_trans ? g_trans[0] : 0.f) * inv_pixels * mask[n * hw + pix];
        const float dden = div_sq(-g * p.E, p.den);
        float de[3], ds[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            de[i] = g * 2.0f * p.e[i] / p.den;
            d_tA[((long)n * 3 + i) * hw + pix] = de[i] + dden * 2.0f * p.tA[i];
        }
        const Taps& t = p.t4;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            ds[j] = (R[j] * de[0] + R[3 + j] * de[1] + R[6 + j] * de[2]) + dden * 2.0f * p.s[j];
#pragma unroll
            for (int i = 0; i < 3; ++i) acc9[3 * i + j] = de[i] * p.s[j];
            // grid_sample's own backward: scatter through the four taps (zeros padding: taps outside receive nothing); fp32 vector atomics
            float* pl = d_tB + ((long)n * 3 + j) * hw;
            if (t.okx0 && t.oky0) unsafeAtomicAdd(pl + (long)t.y0 * W + t.x0, ds[j] * (t.sy * t.ex));
            if (t.okx1 && t.oky0) unsafeAtomicAdd(pl + (long)t.y0 * W + t.x0 + 1, ds[j] * (t.sy * t.wx));
            if (t.okx0 && t.oky1) unsafeAtomicAdd(pl + (long)(t.y0 + 1) * W + t.x0, ds[j] * (t.ny * t.ex));
            if (t.okx1 && t.oky1) unsafeAtomicAdd(pl + (long)(t.y0 + 1) * W + t.x0 + 1, ds[j] * (t.ny * t.wx));
        }
    }
    const int blk = (n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    sde_block_sums<9, PB_N / 64>(acc9, red, dR_partial + 9 * (long)blk);
}

// d R_A2B = sum of the translation term's partials + rotation term, d R_B2A = rotation term: one wave per sample
__global__ void __launch_bounds__(64) mc_bwd_finalize_kernel(const float* __restrict__ partial, int bps, const float* __restrict__ R1, const float* __restrict__ R2,
                                                             const float* __restrict__ g_rot, int N, float* __restrict__ dR1, float* __restrict__ dR2) {
    const int n = blockIdx.x, lane = threadIdx.x;
    float acc[9];
    sample_sum9(partial, n, bps, acc);
    if (lane == 0) {
        float a[9], b[9];
        mc_rot(R1 + 9 * n, R2 + 9 * n, (g_rot ? g_rot[0] : 0.f) / (float)N, a, b);
#pragma unroll
        for (int i = 0; i < 9; ++i) { dR1[n * 9 + i] = acc[i] + a[i]; dR2[n * 9 + i] = b[i]; }
    }
}

// ------------------------------------------------------------------------------------------------
// motion_smoothness_loss_fn / motion_sparsity_loss_fn (motion_loss.py:L51-64).  One launch forward: per-workgroup partials, and the workgroup that
// arrives last (device-scope ticket, left at zero again) adds them up in index order.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ticket_finalize(float s, float* __restrict__ partial, int nblk, int blk, float scale, float* __restrict__ out, int* __restrict__ ticket) {
    if (threadIdx.x == 0) __hip_atomic_store(partial + blk, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (sde_arrive_last(ticket, nblk) && threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < nblk; ++i) t += ld_agent(partial + i);
        out[0] = t * scale;
    }
}

// element (i, j), i < H-1, j < W-1:  gx = f[i+1][j+1] - f[i+1][j],  gy = f[i+1][j+1] - f[i][j+1]  (the reversed gradients, cropped by one row / column)
__global__ void __launch_bounds__(PB_N) msmooth_fwd_kernel(const float* __restrict__ f, int planes, int H, int W, float scale, float* __restrict__ partial,
                                                           float* __restrict__ out, int* __restrict__ ticket) {
    __shared__ float red[16];
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    float v = 0.f;
    if (i < H - 1 && j < W - 1)
        for (int p = blockIdx.z; p < planes; p += gridDim.z) {
            const float* s = f + (long)p * H * W;
            const float c = s[(long)(i + 1) * W + j + 1], gx = c - s[(long)(i + 1) * W + j], gy = c - s[(long)i * W + j + 1];
            v += sqrtf(1e-24f + gx * gx + gy * gy);
        }
    const float s = sde_block_sum(v, red);
    const int nblk = gridDim.x * gridDim.y * gridDim.z, blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    ticket_finalize(s, partial, nblk, blk, scale, out, ticket);
}

__global__ void __launch_bounds__(PB_N) msmooth_bwd_kernel(const float* __restrict__ f, const float* __restrict__ gout, int planes, int H, int W, float scale,
                                                           float* __restrict__ df) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float g = gout[0] * scale;
    for (int p = blockIdx.z; p < planes; p += gridDim.z) {
        const float* s = f + (long)p * H * W;
        auto elem = [&](int i, int j, float& gx, float& gy, float& r) {
            const float c = s[(long)(i + 1) * W + j + 1];
            gx = c - s[(long)(i + 1) * W + j]; gy = c - s[(long)i * W + j + 1];
            r = 1.0f / sqrtf(1e-24f + gx * gx + gy * gy);
        };
        float d = 0.f, gx, gy, r;
        if (y >= 1 && x >= 1) { elem(y - 1, x - 1, gx, gy, r); d += (gx + gy) * r; }      // this pixel is the element's corner f[i+1][j+1]
        if (y >= 1 && x <= W - 2) { elem(y - 1, x, gx, gy, r); d -= gx * r; }              // ... its f[i+1][j]
        if (y <= H - 2 && x >= 1) { elem(y, x - 1, gx, gy, r); d -= gy * r; }              // ... its f[i][j+1]
        df[(long)p * H * W + (long)y * W + x] = g * d;
    }
}

// one workgroup per plane: mean |f| (kept for the backward), then sum 2 m sqrt(|f| / (m + 1e-24) + 1)
__global__ void __launch_bounds__(1024) msparse_fwd_kernel(const float* __restrict__ f, int planes, long hw, float scale, float* __restrict__ mean, float* __restrict__ partial,
                                                           float* __restrict__ out, int* __restrict__ ticket) {
    __shared__ float red[16];
    __shared__ float ms;
    const int p = blockIdx.x;
    const float* s = f + (long)p * hw;
    float v = 0.f;
    for (long i = threadIdx.x; i < hw; i += 1024) v += fabsf(s[i]);
    v = sde_block_sum(v, red);
    if (threadIdx.x == 0) { ms = v / (float)hw; mean[p] = ms; }
    __syncthreads();
    const float m = ms, rm = 1.0f / (m + 1e-24f);
    v = 0.f;
    for (long i = threadIdx.x; i < hw; i += 1024) v += (2.0f * m) * sqrtf(fabsf(s[i]) * rm + 1.0f);
    v = sde_block_sum(v, red);
    ticket_finalize(v, partial, planes, p, scale, out, ticket);
}

__global__ void __launch_bounds__(PB_N) msparse_bwd_kernel(const float* __restrict__ f, const float* __restrict__ mean, const float* __restrict__ gout, long hw, float scale,
                                                           float* __restrict__ df) {
    const int p = blockIdx.y;
    const long i = (long)blockIdx.x * PB_N + threadIdx.x;
    if (i >= hw) return;
    const float m = mean[p], rm = 1.0f / (m + 1e-24f), v = f[(long)p * hw + i];
    const float sg = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
    df[(long)p * hw + i] = gout[0] * scale * m * rm * sg / sqrtf(fabsf(v) * rm + 1.0f);
}

// ------------------------------------------------------------------------------------------------
// resize_img_avgpool = F.adaptive_avg_pool2d (camera.py:L49-54): window [floor(i H / h), ceil((i + 1) H / h))
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ap_lo(int i, int H, int h) { return (int)(((long)i * H) / h); }
__device__ __forceinline__ int ap_hi(int i, int H, int h) { return (int)(((long)(i + 1) * H + h - 1) / h); }

__global__ void __launch_bounds__(PB_N) avgpool_fwd_kernel(const float* __restrict__ src, float* __restrict__ dst, int planes, int H, int W, int h, int w) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int y0 = ap_lo(y, H, h), y1 = ap_hi(y, H, h), x0 = ap_lo(x, W, w), x1 = ap_hi(x, W, w);
    const float inv = 1.0f / (float)((y1 - y0) * (x1 - x0));
    for (int p = blockIdx.z; p < planes; p += gridDim.z) {
        const float* s = src + (long)p * H * W;
        float acc = 0.f;
        for (int yy = y0; yy < y1; ++yy)
            for (int xx = x0; xx < x1; ++xx) acc += s[(long)yy * W + xx];
        dst[((long)p * h + y) * w + x] = acc * inv;
    }
}

// the output rows whose window contains input row y are contiguous and include floor(y h / H)
__device__ __forceinline__ void ap_range(int y, int H, int h, int& lo, int& hi) {
    lo = hi = (int)(((long)y * h) / H);
    while (lo > 0 && ap_hi(lo - 1, H, h) > y) --lo;
    while (hi + 1 < h && ap_lo(hi + 1, H, h) <= y) ++hi;
}

__global__ void __launch_bounds__(PB_N) avgpool_bwd_kernel(const float* __restrict__ dout, float* __restrict__ din, int planes, int H, int W, int h, int w) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    int i0, i1, j0, j1;
    ap_range(y, H, h, i0, i1);
    ap_range(x, W, w, j0, j1);
    for (int p = blockIdx.z; p < planes; p += gridDim.z) {
        const float* s = dout + (long)p * h * w;
        float acc = 0.f;
        for (int i = i0; i <= i1; ++i) {
            const float ry = 1.0f / (float)(ap_hi(i, H, h) - ap_lo(i, H, h));
            for (int j = j0; j <= j1; ++j) acc += s[(long)i * w + j] * (ry / (float)(ap_hi(j, W, w) - ap_lo(j, W, w)));
        }
        din[((long)p * H + y) * W + x] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
// Per-scale glue of MotionLearningModel between the networks and the loss operators (MotionLearning.py:L126-166, L205-208), both directions stacked
// along the batch (N = 2B).  Forward: prep_pool_kernel (pools, t = t_pose + m_r, per-workgroup sums of depth_r and t^2), prep_fwd_finalize_kernel (one
// workgroup per sample adds them up; the one that arrives last forms the batch depth mean and the per-sample motion scale) and prep_scale_kernel (the
// divisions and the half-swapped copies).  Backward: prep_bwd_reduce_kernel (the dot products behind d mean, d scale and d t_pose),
// prep_bwd_finalize_kernel and prep_bwd_gather_kernel (pool transposed).
// stats [2 + 4N]: depth_mean, 1 / depth_mean, sqrt(3 mean t^2 + 1e-12) [N], 3 mean t^2 [N], scratch [N][2].  No float atomics: every sum has a fixed order.
// ------------------------------------------------------------------------------------------------
struct PrepArgs {
    const float *__restrict__ depth, *__restrict__ motion, *__restrict__ tpose, *__restrict__ mask;      // motion, mask: may be null
    int N, H0, W0, h, w, normalize;
    float *__restrict__ depth_r, *__restrict__ t0, *__restrict__ m_r;      // t0 = t_pose + m_r; m_r [N,3,h,w] (null without motion)
    float *partial, *stats;                          // [workgroups][2], [2 + 4N]
    int* ticket;                                     // one int, zero between launches
};

// Finalize kernels (one workgroup per sample, launched after the pass that wrote the partials): the workgroup adds its sample's NV partials up (256
// threads stride the workgroups of the pass, then the block sum: fixed order), publishes them to per[n][NV] and counts on the ticket; true in every thread
// of the workgroup that arrives last, which then does the part that needs all samples.  The arrival is kept out of the passes themselves: counting their
// 7168 workgroups on one address cost 0.7 ms per launch, and on one address per sample still 0.2 ms (profiles/motion_prep_kernels.txt).
template <int NV>
__device__ __forceinline__ bool sample_sums_and_arrive(float* sums /*LDS [NV]*/, float* red /*LDS [4 * NV]*/, const float* __restrict__ partial, float* __restrict__ per,
                                                       int n, int N, int bps, int* __restrict__ ticket) {
    float v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.f;
    sde_partial_walk<NV, PB_N>(v, partial, (long)n * bps, bps, threadIdx.x);
    sde_block_sums<NV, PB_N / 64>(v, red, sums);
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) __hip_atomic_store(per + (long)n * NV + k, sums[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return sde_arrive_last(ticket, N);
}

__global__ void __launch_bounds__(PB_N) prep_pool_kernel(const PrepArgs a) {
    __shared__ float red[8];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    const int H0 = a.H0, W0 = a.W0, h = a.h, w = a.w;
    float v[2] = {0.f, 0.f};
    if (x < w && y < h) {
        const int y0 = ap_lo(y, H0, h), y1 = ap_hi(y, H0, h), x0 = ap_lo(x, W0, w), x1 = ap_hi(x, W0, w);
        const float inv = 1.0f / (float)((y1 - y0) * (x1 - x0));
        const float* d = a.depth + (long)n * H0 * W0;
        const float* k = a.mask ? a.mask + (long)n * H0 * W0 : nullptr;
        float acc = 0.f;
        for (int yy = y0; yy < y1; ++yy)
            for (int xx = x0; xx < x1; ++xx) acc += d[(long)yy * W0 + xx];
        const long o = ((long)n * h + y) * w + x;
        v[0] = acc * inv;
        a.depth_r[o] = v[0];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long oc = (((long)n * 3 + c) * h + y) * w + x;
            float t = a.tpose[n * 3 + c];
            if (a.motion) {
                const float* m = a.motion + ((long)n * 3 + c) * H0 * W0;
                acc = 0.f;
                for (int yy = y0; yy < y1; ++yy)
                    for (int xx = x0; xx < x1; ++xx) acc += k ? m[(long)yy * W0 + xx] * k[(long)yy * W0 + xx] : m[(long)yy * W0 + xx];
                const float mr = acc * inv;
                a.m_r[oc] = mr;
                t = t + mr;
            }
            a.t0[oc] = t;
            v[1] += t * t;
        }
    }
    sde_block_sums<2, PB_N / 64>(v, red, a.partial + 2 * (long)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x));
}

// depth mean and per-sample motion scale from the partials of prep_pool_kernel: grid N
__global__ void __launch_bounds__(PB_N) prep_fwd_finalize_kernel(const PrepArgs a, int bps) {
    __shared__ float red[8], sums[2];
    const int n = blockIdx.x, N = a.N, h = a.h, w = a.w;
    float* per = a.stats + 2 + 2 * N;                     // scratch [N][2]: sum depth_r, sum t0^2 of each sample
    if (!sample_sums_and_arrive<2>(sums, red, a.partial, per, n, N, bps, a.ticket)) return;
    // the workgroup that arrives last of all: depth mean over the samples in a fixed order (thread-strided, then the block sum), then one thread per sample
    __shared__ float mu_s;
    const float hw = (float)h * (float)w;
    float s = 0.f;
    if (a.normalize)
        for (int i = threadIdx.x; i < N; i += PB_N) s += ld_agent(per + 2 * i);
    s = sde_block_sum(s, red);
    if (threadIdx.x == 0) {
        mu_s = a.normalize ? s / ((float)N * hw) : 1.0f;
        a.stats[0] = mu_s;
        a.stats[1] = 1.0f / mu_s;
    }
    __syncthreads();
    const float mu = mu_s;
    for (int i = threadIdx.x; i < N; i += PB_N) {
        const float q = ld_agent(per + 2 * i + 1) / (mu * mu) / hw;       // 3 mean_{c,h,w}(t^2) with t = t0 / mu
        a.stats[2 + N + i] = q;
        a.stats[2 + i] = sqrtf(q + 1e-12f);
    }
}

// depth_n = depth_r / mean, t = t0 / mean, m_norm = (m_r / mean) / sqrt(3 mean t^2 + 1e-12) (in place over m_r), and the copies of depth_n and t with the two
// halves of the batch exchanged (depth_B of the stacked RGB-D call, t_B2A of motion consistency).  Without normalisation depth_n is depth_r and t is t0.
__global__ void __launch_bounds__(PB_N) prep_scale_kernel(const float* __restrict__ depth_r, const float* __restrict__ t0, const float* __restrict__ stats,
                                                          int N, int h, int w, int normalize, float* __restrict__ depth_n, float* __restrict__ t,
                                                          float* __restrict__ m, float* __restrict__ depth_n_sw, float* __restrict__ t_sw) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    if (x >= w || y >= h) return;
    const int ns = n < N / 2 ? n + N / 2 : n - N / 2;
    const float mu = stats[0], sq = stats[2 + n];
    const long pix = (long)y * w + x, hw = (long)h * w;
    float dn = depth_r[n * hw + pix];
    if (normalize) { dn = dn / mu; depth_n[n * hw + pix] = dn; }
    if (depth_n_sw) depth_n_sw[ns * hw + pix] = dn;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long o = ((long)n * 3 + c) * hw + pix;
        float tv = t0[o];
        if (normalize) { tv = tv / mu; t[o] = tv; }
        if (t_sw) t_sw[((long)ns * 3 + c) * hw + pix] = tv;
        if (m) {
            float mv = m[o];
            if (normalize) mv = mv / mu;
            m[o] = mv / sq;
        }
    }
}

struct PrepBwdArgs {
    const float *mask, *depth_n, *t, *m_norm, *stats;                      // mask, m_norm: may be null
    const float *g_depth_r, *g_depth_n, *g_t, *g_t_sw, *g_m_norm;          // each may be null (= zero)
    int N, H0, W0, h, w, normalize;
    float *partial, *bstats;                                               // [workgroups][9], [1 + 10N]: d mean per pooled pixel, c [N], scratch [N][9]
    int* ticket;                                                           // one int, zero between launches
    float *d_depth, *d_motion, *d_tpose;                                   // d_motion: null without motion
};

// d loss / d t of one pooled element: the direct gradient plus the one that arrives through the half-swapped copy
__device__ __forceinline__ float prep_gt(const PrepBwdArgs& a, long o, long o_sw) {
    float g = 0.f;
    if (a.g_t) g = a.g_t[o];
    if (a.g_t_sw) g += a.g_t_sw[o_sw];
    return g;
}

// per sample: A = sum g_m_norm m_norm, Bt = sum g_t t, C = sum g_depth_n depth_n, sum g_t [3], sum t [3]; prep_bwd_finalize_kernel forms
// c_n = -A / ((3 mean t^2 + 1e-12) h w)  (so that d t = g_t + c_n t), d t_pose and d depth_mean
__global__ void __launch_bounds__(PB_N) prep_bwd_reduce_kernel(const PrepBwdArgs a) {
    __shared__ float red[36];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    const int h = a.h, w = a.w, N = a.N;
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (x < w && y < h) {
        const int ns = n < N / 2 ? n + N / 2 : n - N / 2;
        const long pix = (long)y * w + x, hw = (long)h * w;
        if (a.g_depth_n) v[2] = a.g_depth_n[n * hw + pix] * a.depth_n[n * hw + pix];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long o = ((long)n * 3 + c) * hw + pix;
            const float g = prep_gt(a, o, ((long)ns * 3 + c) * hw + pix), tv = a.t[o];
            if (a.m_norm && a.g_m_norm) v[0] += a.g_m_norm[o] * a.m_norm[o];
            v[1] += g * tv;
            v[3 + c] = g;
            v[6 + c] = tv;
        }
    }
    sde_block_sums<9, PB_N / 64>(v, red, a.partial + 9 * (long)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x));
}

// c_n, d t_pose and d depth_mean from the partials of prep_bwd_reduce_kernel: grid N
__global__ void __launch_bounds__(PB_N) prep_bwd_finalize_kernel(const PrepBwdArgs a, int bps) {
    __shared__ float red[36], sums[9];
    const int n = blockIdx.x, N = a.N, h = a.h, w = a.w;
    float* per = a.bstats + 1 + N;
    if (!sample_sums_and_arrive<9>(sums, red, a.partial, per, n, N, bps, a.ticket)) return;
    const float hw = (float)h * (float)w, r = a.normalize ? a.stats[1] : 1.0f;
    float tot = 0.f;
    for (int i = threadIdx.x; i < N; i += PB_N) {         // one thread per sample; d depth_mean: thread-strided, then the block sum
        float p[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) p[k] = ld_agent(per + 9 * i + k);
        const float sq = a.stats[2 + i], s = a.stats[2 + N + i];
        const float cn = a.m_norm ? -p[0] / (sq * sq) / hw : 0.f;
        a.bstats[1 + i] = cn;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.d_tpose[i * 3 + c] = r * (p[3 + c] + cn * p[6 + c]);
        tot += ((p[1] + cn * (s * hw)) + p[0]) + p[2];
    }
    tot = sde_block_sum(tot, red);
    if (threadIdx.x == 0) a.bstats[0] = a.normalize ? (-r * tot) / ((float)N * hw) : 0.f;
}

// d depth and d motion of one full-resolution pixel: the pooled gradients of the windows that contain it (a contiguous range each way), over the window areas
__global__ void __launch_bounds__(PB_N) prep_bwd_gather_kernel(const PrepBwdArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
    const int H0 = a.H0, W0 = a.W0, h = a.h, w = a.w, N = a.N;
    if (x >= W0 || y >= H0) return;
    int i0, i1, j0, j1;
    ap_range(y, H0, h, i0, i1);
    ap_range(x, W0, w, j0, j1);
    const int ns = n < N / 2 ? n + N / 2 : n - N / 2;
    const long hw = (long)h * w;
    const float r = a.normalize ? a.stats[1] : 1.0f, gmu = a.bstats[0], cn = a.bstats[1 + n];
    const float rs = 1.0f / a.stats[2 + n];
    const bool motion = a.d_motion != nullptr;
    float dd = 0.f, dm[3] = {0.f, 0.f, 0.f};
    for (int i = i0; i <= i1; ++i) {
        const float ry = 1.0f / (float)(ap_hi(i, H0, h) - ap_lo(i, H0, h));
        for (int j = j0; j <= j1; ++j) {
            const float wgt = ry / (float)(ap_hi(j, W0, w) - ap_lo(j, W0, w));
            const long pix = (long)i * w + j;
            float g = gmu;
            if (a.g_depth_r) g += a.g_depth_r[n * hw + pix];
            if (a.g_depth_n) g += a.g_depth_n[n * hw + pix] * r;
            dd += g * wgt;
            if (motion) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const long o = ((long)n * 3 + c) * hw + pix;
                    float gm = prep_gt(a, o, ((long)ns * 3 + c) * hw + pix) + cn * a.t[o];
                    if (a.g_m_norm) gm += a.g_m_norm[o] * rs;
                    dm[c] += (r * gm) * wgt;
                }
            }
        }
    }
    const long o = (long)y * W0 + x, HW0 = (long)H0 * W0;
    a.d_depth[n * HW0 + o] = dd;
    if (motion) {
        const float k = a.mask ? a.mask[n * HW0 + o] : 1.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.d_motion[((long)n * 3 + c) * HW0 + o] = dm[c] * k;
    }
}

// ------------------------------------------------------------------------------------------------
// Mask dilation: max_pool2d(mask > 0, 2d + 1, stride 1, padding d) as a row pass and a column pass of 2d + 1 taps each (clipped to the image)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PB_N) dilate_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W, int d, int horizontal) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const float* s = src + (long)blockIdx.z * H * W;
    bool on = false;
    if (horizontal) {
        const int lo = x - d > 0 ? x - d : 0, hi = x + d < W - 1 ? x + d : W - 1;
        for (int xx = lo; xx <= hi; ++xx) on = on || s[(long)y * W + xx] > 0.f;
    } else {
        const int lo = y - d > 0 ? y - d : 0, hi = y + d < H - 1 ? y + d : H - 1;
        for (int yy = lo; yy <= hi; ++yy) on = on || s[(long)yy * W + x] > 0.f;
    }
    dst[(long)blockIdx.z * H * W + (long)y * W + x] = on ? 1.0f : 0.f;
}

inline dim3 pix_grid(int W, int H, int z) { return dim3(sde_cdiv(W, 64), sde_cdiv(H, 4), z); }
inline int ssim_mode(float C1, float C2) { return C1 > kFltMax ? 1 : (C2 > kFltMax ? 2 : 0); }
constexpr int kMaxZ = 65535;

}  // namespace

extern "C" {

int sde_view_synthesis_pp(const float* img, const float* depth, const float* K, const float* R, const float* t, int B, int C, int H, int W, float* sampled,
                          float* Z, float* grid, uint8_t* valid, sde_stream_t stream) {
    SDE_CHECK_ARG(img && depth && K && R && t && sampled, "sde_view_synthesis_pp: null pointer");
    SDE_CHECK_ARG(B > 0 && B <= kMaxZ && C > 0 && H > 1 && W > 1, "sde_view_synthesis_pp: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    hipLaunchKernelGGL(view_synthesis_pp_kernel, pix_grid(W, H, B), dim3(PB_N), 0, (hipStream_t)stream, img, depth, K, R, t, C, H, W, sampled, Z, grid, valid);
    SDE_CHECK_LAUNCH("sde_view_synthesis_pp");
    return SDE_OK;
}

int sde_rgbd_num_blocks(int N, int H, int W) { return N * sde_cdiv(W, 64) * sde_cdiv(H, 4); }

int sde_rgbd_fwd(const sde_rgbd_desc* d, float* sampled, float* grid, float* occ, float* err, uint8_t* valid, float* dpw, float* part1, float* part2,
                 float* stats, sde_stream_t stream) {
    SDE_CHECK_ARG(d && d->frame_A && d->frame_B && d->depth_A && d->depth_B && d->K && d->R && d->t, "sde_rgbd_fwd: null input");
    SDE_CHECK_ARG(sampled && grid && occ && err && valid && part1 && stats, "sde_rgbd_fwd: null output");
    SDE_CHECK_ARG(d->N > 0 && d->N <= kMaxZ && d->H > 1 && d->W > 1, "sde_rgbd_fwd: bad shape N=%d H=%d W=%d", d->N, d->H, d->W);
    SDE_CHECK_ARG(!d->ssim || (dpw && part2), "sde_rgbd_fwd: SSIM term without its buffers");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g = pix_grid(d->W, d->H, d->N);
    RgbdArgs a{d->frame_A, d->frame_B, d->depth_A, d->depth_B, d->K, d->R, d->t, d->N, d->H, d->W, sampled, grid, occ, err, valid, part1};
    hipLaunchKernelGGL(rgbd_warp_kernel, g, dim3(PB_N), 0, st, a);
    SDE_CHECK_LAUNCH("sde_rgbd_fwd/warp");
    if (d->ssim) {
        WssimArgs w{sampled, d->frame_A, nullptr, err, valid, part1, d->N, 3, d->H, d->W, ssim_mode(d->C1, d->C2), d->C1, d->C2, nullptr, nullptr, dpw, part2};
        hipLaunchKernelGGL(wssim_fwd_kernel, g, dim3(PB_N), 0, st, w);
        SDE_CHECK_LAUNCH("sde_rgbd_fwd/ssim");
    }
    hipLaunchKernelGGL(rgbd_finalize_kernel, dim3(d->N), dim3(PB_N), 0, st, (const float*)part1, (const float*)(d->ssim ? part2 : nullptr), (int)(g.x * g.y), d->N, stats);
    SDE_CHECK_LAUNCH("sde_rgbd_fwd/finalize");
    return SDE_OK;
}

int sde_rgbd_bwd(const sde_rgbd_desc* d, const float* sampled, const float* occ, const float* err, const float* dpw, const float* stats, const float* g_l1,
                 const float* g_ssim, const float* g_dl1, float gscale_ssim, float* coef, float* d_depth, float* d_t, float* dR_partial, float* dR,
                 sde_stream_t stream) {
    SDE_CHECK_ARG(d && d->frame_A && d->frame_B && d->depth_A && d->K && d->R && d->t, "sde_rgbd_bwd: null input");
    SDE_CHECK_ARG(sampled && occ && err && stats && d_depth && d_t && dR_partial && dR, "sde_rgbd_bwd: null pointer");
    SDE_CHECK_ARG(d->N > 0 && d->N <= kMaxZ && d->H > 1 && d->W > 1, "sde_rgbd_bwd: bad shape N=%d H=%d W=%d", d->N, d->H, d->W);
    const bool ssim = d->ssim && g_ssim;
    SDE_CHECK_ARG(!ssim || (dpw && coef), "sde_rgbd_bwd: SSIM term without its buffers");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g = pix_grid(d->W, d->H, d->N);
    if (ssim) {
        WssimArgs w{sampled, d->frame_A, dpw, nullptr, nullptr, nullptr, d->N, 3, d->H, d->W, ssim_mode(d->C1, d->C2), d->C1, d->C2, nullptr, nullptr, nullptr, nullptr};
        hipLaunchKernelGGL(wssim_coef_kernel, g, dim3(PB_N), 0, st, w, (const float*)nullptr, g_ssim, gscale_ssim, coef);
        SDE_CHECK_LAUNCH("sde_rgbd_bwd/coef");
    }
    RgbdBwdArgs a{d->frame_A, d->frame_B, d->depth_A, d->K, d->R, d->t, sampled, occ, err, dpw, ssim ? coef : nullptr, stats, g_l1, g_dl1,
                  d->N, d->H, d->W, d_depth, d_t, dR_partial};
    hipLaunchKernelGGL(rgbd_bwd_kernel, g, dim3(PB_N), 0, st, a);
    SDE_CHECK_LAUNCH("sde_rgbd_bwd/pixels");
    hipLaunchKernelGGL(sum9_finalize_kernel, dim3(d->N), dim3(64), 0, st, (const float*)dR_partial, (int)(g.x * g.y), dR);
    SDE_CHECK_LAUNCH("sde_rgbd_bwd/finalize");
    return SDE_OK;
}

int sde_wssim_fwd(const float* x, const float* y, const float* w, int N, int C, int H, int W, float C1, float C2, float* map, float* avg_w, sde_stream_t stream) {
    SDE_CHECK_ARG(x && y && w && map && avg_w, "sde_wssim_fwd: null pointer");
    SDE_CHECK_ARG(N > 0 && N <= kMaxZ && C > 0 && H > 1 && W > 1, "sde_wssim_fwd: bad shape N=%d C=%d H=%d W=%d", N, C, H, W);
    WssimArgs a{x, y, w, nullptr, nullptr, nullptr, N, C, H, W, ssim_mode(C1, C2), C1, C2, map, avg_w, nullptr, nullptr};
    hipLaunchKernelGGL(wssim_fwd_kernel, pix_grid(W, H, N), dim3(PB_N), 0, (hipStream_t)stream, a);
    SDE_CHECK_LAUNCH("sde_wssim_fwd");
    return SDE_OK;
}

int sde_wssim_bwd(const float* x, const float* y, const float* w, const float* gout, int N, int C, int H, int W, float C1, float C2, float* coef, float* dx,
                  float* dy, sde_stream_t stream) {
    SDE_CHECK_ARG(x && y && w && gout && coef && (dx || dy), "sde_wssim_bwd: null pointer");
    SDE_CHECK_ARG(N > 0 && N <= kMaxZ && C > 0 && H > 1 && W > 1, "sde_wssim_bwd: bad shape N=%d C=%d H=%d W=%d", N, C, H, W);
    SDE_CHECK_ARG((reinterpret_cast<uintptr_t>(coef) & 15) == 0, "sde_wssim_bwd: coef must be 16-byte aligned");
    WssimArgs a{x, y, w, nullptr, nullptr, nullptr, N, C, H, W, ssim_mode(C1, C2), C1, C2, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(wssim_coef_kernel, pix_grid(W, H, N), dim3(PB_N), 0, (hipStream_t)stream, a, gout, (const float*)nullptr, 0.f, coef);
    SDE_CHECK_LAUNCH("sde_wssim_bwd/coef");
    hipLaunchKernelGGL(wssim_gather_kernel, pix_grid(W, H, N), dim3(PB_N), 0, (hipStream_t)stream, x, y, w, (const float*)coef, C, H, W, dx, dy);
    SDE_CHECK_LAUNCH("sde_wssim_bwd/gather");
    return SDE_OK;
}

int sde_motion_consistency_fwd(const float* grid, const float* mask, const float* R_A2B, const float* R_B2A, const float* t_A2B, const float* t_B2A, int N, int H,
                               int W, float* partial, float* out, sde_stream_t stream) {
    SDE_CHECK_ARG(grid && mask && R_A2B && R_B2A && t_A2B && t_B2A && partial && out, "sde_motion_consistency_fwd: null pointer");
    SDE_CHECK_ARG(N > 0 && N <= kMaxZ && H > 1 && W > 1, "sde_motion_consistency_fwd: bad shape N=%d H=%d W=%d", N, H, W);
    const dim3 g = pix_grid(W, H, N);
    hipLaunchKernelGGL(mc_fwd_kernel, g, dim3(PB_N), 0, (hipStream_t)stream, grid, mask, R_A2B, t_A2B, t_B2A, H, W, partial);
    SDE_CHECK_LAUNCH("sde_motion_consistency_fwd/pixels");
    hipLaunchKernelGGL(mc_finalize_kernel, dim3(1), dim3(PB_N), 0, (hipStream_t)stream, (const float*)partial, (int)(g.x * g.y * g.z), R_A2B, R_B2A, N,
                       1.0f / ((float)N * (float)H * (float)W), out);
    SDE_CHECK_LAUNCH("sde_motion_consistency_fwd/finalize");
    return SDE_OK;
}

int sde_motion_consistency_bwd(const float* grid, const float* mask, const float* R_A2B, const float* R_B2A, const float* t_A2B, const float* t_B2A,
                               const float* g_rot, const float* g_trans, int N, int H, int W, float* d_tA, float* d_tB_zeroed, float* dR_partial, float* dR_A2B,
                               float* dR_B2A, sde_stream_t stream) {
    SDE_CHECK_ARG(grid && mask && R_A2B && R_B2A && t_A2B && t_B2A && d_tA && d_tB_zeroed && dR_partial && dR_A2B && dR_B2A, "sde_motion_consistency_bwd: null pointer");
    SDE_CHECK_ARG(N > 0 && N <= kMaxZ && H > 1 && W > 1, "sde_motion_consistency_bwd: bad shape N=%d H=%d W=%d", N, H, W);
    const dim3 g = pix_grid(W, H, N);
    hipLaunchKernelGGL(mc_bwd_kernel, g, dim3(PB_N), 0, (hipStream_t)stream, grid, mask, R_A2B, t_A2B, t_B2A, g_trans, 1.0f / ((float)N * (float)H * (float)W), H, W,
                       d_tA, d_tB_zeroed, dR_partial);
    SDE_CHECK_LAUNCH("sde_motion_consistency_bwd/pixels");
    hipLaunchKernelGGL(mc_bwd_finalize_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, (const float*)dR_partial, (int)(g.x * g.y), R_A2B, R_B2A, g_rot, N, dR_A2B,
                       dR_B2A);
    SDE_CHECK_LAUNCH("sde_motion_consistency_bwd/finalize");
    return SDE_OK;
}

int sde_motion_smooth_num_blocks(int planes, int H, int W) { return sde_cdiv(W - 1, 64) * sde_cdiv(H - 1, 4) * (planes < 8 ? planes : 8); }

int sde_motion_smooth_fwd(const float* f, int planes, int H, int W, float* partial, float* out, int* ticket, sde_stream_t stream) {
    SDE_CHECK_ARG(f && partial && out && ticket, "sde_motion_smooth_fwd: null pointer");
    SDE_CHECK_ARG(planes > 0 && H > 1 && W > 1, "sde_motion_smooth_fwd: bad shape planes=%d H=%d W=%d", planes, H, W);
    const float scale = 1.0f / ((float)planes * (float)(H - 1) * (float)(W - 1));
    hipLaunchKernelGGL(msmooth_fwd_kernel, pix_grid(W - 1, H - 1, planes < 8 ? planes : 8), dim3(PB_N), 0, (hipStream_t)stream, f, planes, H, W, scale, partial, out, ticket);
    SDE_CHECK_LAUNCH("sde_motion_smooth_fwd");
    return SDE_OK;
}

int sde_motion_smooth_bwd(const float* f, const float* gout, int planes, int H, int W, float* df, sde_stream_t stream) {
    SDE_CHECK_ARG(f && gout && df, "sde_motion_smooth_bwd: null pointer");
    SDE_CHECK_ARG(planes > 0 && H > 1 && W > 1, "sde_motion_smooth_bwd: bad shape planes=%d H=%d W=%d", planes, H, W);
    const float scale = 1.0f / ((float)planes * (float)(H - 1) * (float)(W - 1));
    hipLaunchKernelGGL(msmooth_bwd_kernel, pix_grid(W, H, planes < kMaxZ ? planes : kMaxZ), dim3(PB_N), 0, (hipStream_t)stream, f, gout, planes, H, W, scale, df);
    SDE_CHECK_LAUNCH("sde_motion_smooth_bwd");
    return SDE_OK;
}

int sde_motion_sparsity_fwd(const float* f, int planes, long hw, float* mean, float* partial, float* out, int* ticket, sde_stream_t stream) {
    SDE_CHECK_ARG(f && mean && partial && out && ticket, "sde_motion_sparsity_fwd: null pointer");
    SDE_CHECK_ARG(planes > 0 && hw > 0, "sde_motion_sparsity_fwd: bad shape planes=%d hw=%ld", planes, hw);
    hipLaunchKernelGGL(msparse_fwd_kernel, dim3(planes), dim3(1024), 0, (hipStream_t)stream, f, planes, hw, 1.0f / ((float)planes * (float)hw), mean, partial, out, ticket);
    SDE_CHECK_LAUNCH("sde_motion_sparsity_fwd");
    return SDE_OK;
}

int sde_motion_sparsity_bwd(const float* f, const float* mean, const float* gout, int planes, long hw, float* df, sde_stream_t stream) {
    SDE_CHECK_ARG(f && mean && gout && df, "sde_motion_sparsity_bwd: null pointer");
    SDE_CHECK_ARG(planes > 0 && planes <= kMaxZ && hw > 0, "sde_motion_sparsity_bwd: bad shape planes=%d hw=%ld", planes, hw);
    hipLaunchKernelGGL(msparse_bwd_kernel, dim3(sde_cdiv(hw, PB_N), planes), dim3(PB_N), 0, (hipStream_t)stream, f, mean, gout, hw, 1.0f / ((float)planes * (float)hw), df);
    SDE_CHECK_LAUNCH("sde_motion_sparsity_bwd");
    return SDE_OK;
}

int sde_avgpool_fwd(const float* src, float* dst, int planes, int H, int W, int h, int w, sde_stream_t stream) {
    SDE_CHECK_ARG(src && dst, "sde_avgpool_fwd: null pointer");
    SDE_CHECK_ARG(planes > 0 && H > 0 && W > 0 && h > 0 && w > 0, "sde_avgpool_fwd: bad shape");
    hipLaunchKernelGGL(avgpool_fwd_kernel, pix_grid(w, h, planes < kMaxZ ? planes : kMaxZ), dim3(PB_N), 0, (hipStream_t)stream, src, dst, planes, H, W, h, w);
    SDE_CHECK_LAUNCH("sde_avgpool_fwd");
    return SDE_OK;
}

int sde_avgpool_bwd(const float* dout, float* din, int planes, int H, int W, int h, int w, sde_stream_t stream) {
    SDE_CHECK_ARG(dout && din, "sde_avgpool_bwd: null pointer");
    SDE_CHECK_ARG(planes > 0 && H > 0 && W > 0 && h > 0 && w > 0, "sde_avgpool_bwd: bad shape");
    hipLaunchKernelGGL(avgpool_bwd_kernel, pix_grid(W, H, planes < kMaxZ ? planes : kMaxZ), dim3(PB_N), 0, (hipStream_t)stream, dout, din, planes, H, W, h, w);
    SDE_CHECK_LAUNCH("sde_avgpool_bwd");
    return SDE_OK;
}

int sde_motion_prep_fwd(const float* depth, const float* motion, const float* t_pose, const float* mask01, int N, int H0, int W0, int h, int w, int normalize,
                        float* depth_r, float* depth_n, float* t, float* overall, float* m_norm, float* depth_n_sw, float* t_sw, float* partial, float* stats,
                        int* ticket, sde_stream_t stream) {
    SDE_CHECK_ARG(depth && t_pose && depth_r && t && partial && stats && ticket, "sde_motion_prep_fwd: null pointer");
    SDE_CHECK_ARG(N > 0 && N <= kMaxZ && N % 2 == 0 && H0 > 0 && W0 > 0 && h > 0 && w > 0 && h <= H0 && w <= W0,
                  "sde_motion_prep_fwd: bad shape N=%d (even: both directions stacked) %dx%d -> %dx%d", N, H0, W0, h, w);
    SDE_CHECK_ARG(!normalize || (depth_n && overall), "sde_motion_prep_fwd: scale_normalize without depth_n / overall");
    SDE_CHECK_ARG((motion != nullptr) == (m_norm != nullptr) && (motion || !mask01), "sde_motion_prep_fwd: motion, m_norm and mask01 go together");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g = pix_grid(w, h, N);
    float* t0 = normalize ? overall : t;
    PrepArgs a{depth, motion, t_pose, mask01, N, H0, W0, h, w, normalize ? 1 : 0, depth_r, t0, m_norm, partial, stats, ticket};
    hipLaunchKernelGGL(prep_pool_kernel, g, dim3(PB_N), 0, st, a);
    SDE_CHECK_LAUNCH("sde_motion_prep_fwd/pool");
    hipLaunchKernelGGL(prep_fwd_finalize_kernel, dim3(N), dim3(PB_N), 0, st, a, (int)(g.x * g.y));
    SDE_CHECK_LAUNCH("sde_motion_prep_fwd/finalize");
    if (normalize || m_norm || depth_n_sw || t_sw) {
        hipLaunchKernelGGL(prep_scale_kernel, g, dim3(PB_N), 0, st, (const float*)depth_r, (const float*)t0, (const float*)stats, N, h, w, normalize ? 1 : 0, depth_n, t,
                           m_norm, depth_n_sw, t_sw);
        SDE_CHECK_LAUNCH("sde_motion_prep_fwd/scale");
    }
    return SDE_OK;
}

int sde_motion_prep_bwd(const float* mask01, const float* depth_n, const float* t, const float* m_norm, const float* stats, const float* g_depth_r,
                        const float* g_depth_n, const float* g_t, const float* g_t_sw, const float* g_m_norm, int N, int H0, int W0, int h, int w, int normalize,
                        float* partial, float* bstats, int* ticket, float* d_depth, float* d_motion, float* d_tpose, sde_stream_t stream) {
    SDE_CHECK_ARG(t && stats && partial && bstats && ticket && d_depth && d_tpose, "sde_motion_prep_bwd: null pointer");
    SDE_CHECK_ARG(N > 0 && N <= kMaxZ && N % 2 == 0 && H0 > 0 && W0 > 0 && h > 0 && w > 0 && h <= H0 && w <= W0,
                  "sde_motion_prep_bwd: bad shape N=%d %dx%d -> %dx%d", N, H0, W0, h, w);
    SDE_CHECK_ARG((m_norm != nullptr) == (d_motion != nullptr) && (m_norm || !mask01), "sde_motion_prep_bwd: m_norm, d_motion and mask01 go together");
    SDE_CHECK_ARG(!g_depth_n || (normalize && depth_n), "sde_motion_prep_bwd: a gradient of depth_n without scale_normalize");
    hipStream_t st = (hipStream_t)stream;
    PrepBwdArgs a{mask01, depth_n, t, m_norm, stats, g_depth_r, g_depth_n, g_t, g_t_sw, g_m_norm, N, H0, W0, h, w, normalize ? 1 : 0, partial, bstats, ticket,
                  d_depth, d_motion, d_tpose};
    const dim3 g = pix_grid(w, h, N);
    hipLaunchKernelGGL(prep_bwd_reduce_kernel, g, dim3(PB_N), 0, st, a);
    SDE_CHECK_LAUNCH("sde_motion_prep_bwd/reduce");
    hipLaunchKernelGGL(prep_bwd_finalize_kernel, dim3(N), dim3(PB_N), 0, st, a, (int)(g.x * g.y));
    SDE_CHECK_LAUNCH("sde_motion_prep_bwd/finalize");
    hipLaunchKernelGGL(prep_bwd_gather_kernel, pix_grid(W0, H0, N), dim3(PB_N), 0, st, a);
    SDE_CHECK_LAUNCH("sde_motion_prep_bwd/gather");
    return SDE_OK;
}

int sde_mask_dilate(const float* mask, float* tmp, float* out, int planes, int H, int W, int d, sde_stream_t stream) {
    SDE_CHECK_ARG(mask && tmp && out && tmp != out && tmp != mask, "sde_mask_dilate: null or aliased pointer");
    SDE_CHECK_ARG(planes > 0 && planes <= kMaxZ && H > 0 && W > 0 && d > 0 && d < (1 << 20), "sde_mask_dilate: bad shape planes=%d H=%d W=%d d=%d", planes, H, W, d);
    hipLaunchKernelGGL(dilate_kernel, pix_grid(W, H, planes), dim3(PB_N), 0, (hipStream_t)stream, mask, tmp, H, W, d, 1);
    SDE_CHECK_LAUNCH("sde_mask_dilate/rows");
    hipLaunchKernelGGL(dilate_kernel, pix_grid(W, H, planes), dim3(PB_N), 0, (hipStream_t)stream, (const float*)tmp, out, H, W, d, 0);
    SDE_CHECK_LAUNCH("sde_mask_dilate/columns");
    return SDE_OK;
}

}  // extern "C"
