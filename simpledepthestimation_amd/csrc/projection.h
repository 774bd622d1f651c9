// Projection helpers shared by the geometry kernels (photometric.hip, motion_loss.hip): pinhole back-projection / projection in the reference's fp32
// operation order, the grid_sample tap set and the ReflectionPad2d(1) index map.  Every file that includes this header MUST be compiled with
// -ffp-contract=off (see photometric.hip: floor() of the sample coordinate is bit-exact only with the explicit fmaf / mul / add order kept).
// Not to be merged with pinhole.h: the inference-side operators keep another operation order (lift, move by [R | s], then project with K).
#pragma once
#include "common.h"

namespace {

constexpr float kEps = 1e-6f;
constexpr float kFltMax = 3.402823466e+38f;

__device__ __forceinline__ int reflect_idx(int i, int n) {   // ReflectionPad2d(1) index map
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

struct Cam {
    float ki[9];   // inverse of the scaled intrinsics (camera.py:L25-37)
    float kr[9];   // K @ R   (3x3 @ 3x3: torch naive path, no FMA)
    float kt[3];   // K @ t   (MKL path: mul, fma, fma)
    float k[9];    // scaled intrinsics (camera.py:L14-22)
};

// The camera of a (sample, context) is the same for every lane of a workgroup: moved into scalar registers (v_readfirstlane), its 30 values stop
// occupying vector registers across the projection / VJP code (the backward kernel is register-bound: 120 VGPRs = 4 waves per SIMD with them in VGPRs).
__device__ __forceinline__ float sde_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ Cam cam_uniform(const Cam& c) {
    Cam u;
#pragma unroll
    for (int i = 0; i < 9; ++i) { u.ki[i] = sde_uniform(c.ki[i]); u.kr[i] = sde_uniform(c.kr[i]); u.k[i] = sde_uniform(c.k[i]); }
#pragma unroll
    for (int i = 0; i < 3; ++i) u.kt[i] = sde_uniform(c.kt[i]);
    return u;
}

__device__ __forceinline__ void make_cam(const float* __restrict__ K, const float* __restrict__ P, float sx, float sy,
                                         Cam& c) {
#pragma unroll
    for (int i = 0; i < 9; ++i) c.k[i] = K[i];
    c.k[0] = c.k[0] * sx; c.k[4] = c.k[4] * sy; c.k[2] = c.k[2] * sx; c.k[5] = c.k[5] * sy;
#pragma unroll
    for (int i = 0; i < 9; ++i) c.ki[i] = c.k[i];
    c.ki[0] = 1.0f / c.k[0];
    c.ki[4] = 1.0f / c.k[4];
    c.ki[2] = (-1.0f * c.k[2]) / c.k[0];
    c.ki[5] = (-1.0f * c.k[5]) / c.k[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            c.kr[3 * i + j] = (c.k[3 * i] * P[j] + c.k[3 * i + 1] * P[4 + j]) + c.k[3 * i + 2] * P[8 + j];
        c.kt[i] = fmaf(c.k[3 * i + 2], P[11], fmaf(c.k[3 * i + 1], P[7], c.k[3 * i] * P[3]));
    }
}

struct Proj {
    float p[3];      // back-projected point (camera A)
    float q[3];      // projected homogeneous coords (camera B)
    float X, Y;      // q0/(q2+eps), q1/(q2+eps)
    float ix, iy;    // un-normalised sample coordinate after nan_to_num/clamp/normalise round trip
    bool passx, passy;  // gradient passes nan_to_num + clamp
};

__device__ __forceinline__ float nan_to_num(float v) {
    if (v != v) return 0.f;
    if (v > kFltMax) return kFltMax;
    if (v < -kFltMax) return -kFltMax;
    return v;
}

__device__ __forceinline__ void project(const Cam& c, int x, int y, float d, int W, int H, Proj& o) {
    const float g0 = (float)x * d, g1 = (float)y * d, g2 = d;
#pragma unroll
    for (int i = 0; i < 3; ++i) o.p[i] = fmaf(c.ki[3 * i + 2], g2, fmaf(c.ki[3 * i + 1], g1, c.ki[3 * i] * g0)) + 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        o.q[i] = fmaf(c.kr[3 * i + 2], o.p[2], fmaf(c.kr[3 * i + 1], o.p[1], c.kr[3 * i] * o.p[0])) + c.kt[i];
    const float den = o.q[2] + kEps;
    o.X = o.q[0] / den;
    o.Y = o.q[1] / den;
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    float xs = nan_to_num(o.X), ys = nan_to_num(o.Y);
    o.passx = (o.X == o.X) && (fabsf(o.X) <= kFltMax) && xs >= 0.f && xs <= wm1;
    o.passy = (o.Y == o.Y) && (fabsf(o.Y) <= kFltMax) && ys >= 0.f && ys <= hm1;
    xs = fminf(fmaxf(xs, 0.f), wm1);
    ys = fminf(fmaxf(ys, 0.f), hm1);
    const float xn = (2.0f * xs) / wm1 - 1.0f;
    const float yn = (2.0f * ys) / hm1 - 1.0f;
    o.ix = (xn + 1.0f) * (wm1 / 2.0f);     // ATen CPU grid_sampler un-normalise, align_corners=True
    o.iy = (yn + 1.0f) * (hm1 / 2.0f);
}

struct Taps {
    int x0, y0;
    float wx, ex, ny, sy;   // east/west/north/south weights as in ATen's compute_interp_params
    bool okx0, okx1, oky0, oky1;
};

__device__ __forceinline__ void make_taps(float ix, float iy, int W, int H, Taps& t) {
    const float fx = floorf(ix), fy = floorf(iy);
    t.x0 = (int)fx; t.y0 = (int)fy;
    t.wx = ix - fx; t.ex = 1.0f - t.wx;
    t.ny = iy - fy; t.sy = 1.0f - t.ny;
    t.okx0 = t.x0 >= 0 && t.x0 < W;       t.okx1 = t.x0 + 1 >= 0 && t.x0 + 1 < W;
    t.oky0 = t.y0 >= 0 && t.y0 < H;       t.oky1 = t.y0 + 1 >= 0 && t.y0 + 1 < H;
}

// Bilinear sample of one plane (zeros padding).  Returns value; optionally the 4 tap values.
__device__ __forceinline__ float bilinear(const float* __restrict__ pl, int W, const Taps& t, float* v4) {
    const int x0 = t.x0, y0 = t.y0;
    const float nw = (t.okx0 && t.oky0) ? pl[(long)y0 * W + x0] : 0.f;
    const float ne = (t.okx1 && t.oky0) ? pl[(long)y0 * W + x0 + 1] : 0.f;
    const float sw = (t.okx0 && t.oky1) ? pl[(long)(y0 + 1) * W + x0] : 0.f;
    const float se = (t.okx1 && t.oky1) ? pl[(long)(y0 + 1) * W + x0 + 1] : 0.f;
    if (v4) { v4[0] = nw; v4[1] = ne; v4[2] = sw; v4[3] = se; }
    return nw * (t.sy * t.ex) + ne * (t.sy * t.wx) + sw * (t.ny * t.ex) + se * (t.ny * t.wx);
}

}  // namespace
