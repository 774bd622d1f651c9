// The inference-side pinhole camera, ONE definition for cloud.hip, flow.hip, temporal.hip (and nearest_pixel for lidar.hip): lift a pixel through
// the reference's inv_intrinsics (detectron2/geometry/camera.py L25-37), move it by [R | s], project it again, land on the nearest pixel.  The
// operation order is the one include/sde_hip.h documents and the host twins (hip/twins.py) repeat bit for bit: every file that includes this
// header MUST be compiled with -ffp-contract=off.
// Not to be merged with projection.h: the training path keeps another, reference-dictated operation order (K @ R and K @ t formed first).
#pragma once
#include "common.h"

namespace {

struct Pinhole {
    float fx, cx, fy, cy;            // K[0], K[2], K[4], K[5]
    float k00, k02, k11, k12;        // inv_intrinsics: 1 / fx, (-1 * cx) / fx, 1 / fy, (-1 * cy) / fy
};

__device__ __forceinline__ Pinhole pinhole_load(const float* K) {
    Pinhole c;
    c.fx = K[0]; c.cx = K[2]; c.fy = K[4]; c.cy = K[5];
    c.k00 = 1.f / c.fx; c.k11 = 1.f / c.fy; c.k02 = (-1.f * c.cx) / c.fx; c.k12 = (-1.f * c.cy) / c.fy;
    return c;
}

// pixel (u, v) at depth d -> camera coordinates (px, py, d): five roundings per coordinate, none fused
__device__ __forceinline__ void pinhole_lift(const Pinhole& c, float u, float v, float d, float& px, float& py) {
    px = d * (c.k00 * u + c.k02);
    py = d * (c.k11 * v + c.k12);
}

// q_r = ((R_r0 px + R_r1 py) + R_r2 pz) + s_r; R is row-major with LD floats per row (3: packed, 4: the top of a pose), s = t + m formed by the caller
template <int LD>
__device__ __forceinline__ void pinhole_move(const float* R, float px, float py, float pz, float s0, float s1, float s2, float& qx, float& qy, float& qz) {
    qx = R[0] * px + R[1] * py + R[2] * pz + s0;
    qy = R[LD] * px + R[LD + 1] * py + R[LD + 2] * pz + s1;
    qz = R[2 * LD] * px + R[2 * LD + 1] * py + R[2 * LD + 2] * pz + s2;
}

__device__ __forceinline__ void pinhole_project(const Pinhole& c, float qx, float qy, float qz, float& X, float& Y) {
    const float nx = c.fx * qx + c.cx * qz;
    const float ny = c.fy * qy + c.cy * qz;
    const float den = qz + 1e-6f;
    X = nx / den;
    Y = ny / den;
}

// round-half-even (v_rndne); false beyond any image, which also keeps the int conversion defined (a NaN fails the comparison)
__device__ __forceinline__ bool nearest_pixel(float X, float Y, int& ix, int& iy) {
    constexpr float beyond = 1e9f;
    const float rx = rintf(X), ry = rintf(Y);
    if (!(fabsf(rx) < beyond) || !(fabsf(ry) < beyond)) return false;
    ix = (int)rx;
    iy = (int)ry;
    return true;
}

}  // namespace
