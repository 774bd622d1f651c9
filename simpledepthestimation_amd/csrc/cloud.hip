// Back-projection of depth into 3-D (the reference's detectron2/geometry/camera.py: inv_intrinsics L25-37, img_to_points L125-138), two families.
//
// sde_depth_cloud: the restored metric depth of N frames -> one compacted, coloured point list per frame.  A candidate is a pixel (u, v) with
// u % step == 0 and v % step == 0; candidates are numbered in raster order, q = (v / step) * ceil(W / step) + u / step, and a workgroup owns TILE
// consecutive candidates of one frame, one per thread.  A candidate reads the network output through the index maps of sde_depth_present and is
// kept iff its depth d is finite and min_depth < d <= max_depth.  Stable compaction in three launches, ordered on the stream:
//   cloud_count    kept candidates per workgroup: one __ballot per wave, the four wave counts added by thread 0  -> ws[n][block];
//   cloud_scan     one workgroup per frame walks that frame's counts in chunks of TILE with a running carry: inclusive scan inside a wave by six
//                  __shfl_up steps, the wave totals through LDS; ws[n][block] becomes the exclusive offset, count[n] the total;
//   cloud_scatter  the same decision again (the 4 B per candidate come from cache), rank inside the wave = popcount of the ballot below the lane,
//                  wave bases through LDS, record index = ws[n][block] + wave base + rank.
// No workgroup waits for another, no atomics, placement depends on nothing but the data: the order is the raster order, run after run.
// A record is 16 bytes -- float x, y, z, uint8 r, g, b, a -- and leaves as ONE global_store_dwordx4 (points is 16-byte aligned, checked).  The
// stores of a wave go to consecutive records, so a fully kept wave writes 1 KiB in one piece.
// Per kept candidate: 4 B read twice, 3 B of colour, 16 B written; per dropped one 4 B read twice.
//
// sde_img_to_points_fwd / _bwd: the dense, differentiable img_to_points(depth, R, t), planar [B,3,H,W] fp32.  The backward pass writes ddepth and
// twelve per-workgroup partial sums (dR 9, dt 3); a second launch adds each sample's partials in workgroup order in fp64.  No float atomics.
//
// Built with -ffp-contract=off: the coordinates keep the operation order stated in include/sde_hip.h, which the tests' bound counts.
#include "common.h"
#include "pinhole.h"
#include "sde_hip.h"

namespace {

constexpr int TILE = 256;          // candidates per workgroup = threads per workgroup
constexpr int WAVES = TILE / 64;

struct CloudP {
    const float* pred;           // [N][ph][pw]
    const int* ymap;             // [H]
    const int* xmap;             // [W]
    const uint8_t* frame;        // [N][H][W][3] or null
    const float* K;              // [N][3][3]
    int* ws;                     // [N][nblk]: counts, then exclusive offsets
    int* count;                  // [N]
    uint4* points;               // [N][cap]
    int H, W, ph, pw, step, Wc, cap, nblk;
    float min_depth, max_depth;
};

// candidate q of frame n -> its pixel and restored depth; false past the last candidate
__device__ __forceinline__ bool candidate(const CloudP& p, int n, int q, int& u, int& v, float& d) {
    if (q >= p.cap) return false;
    const int vc = q / p.Wc;
    v = vc * p.step;
    u = (q - vc * p.Wc) * p.step;
    const int r = p.ymap[v], c = p.xmap[u];
    d = (r >= 0 && c >= 0) ? p.pred[((size_t)n * p.ph + r) * p.pw + c] : 0.f;
    return true;
}
__device__ __forceinline__ bool kept(const CloudP& p, float d) {
    return fabsf(d) < INFINITY && p.min_depth < d && d <= p.max_depth;      // NaN fails the first comparison
}

__global__ void __launch_bounds__(TILE) cloud_count(CloudP p) {
    __shared__ int wsum[WAVES];
    const int n = blockIdx.y, q = blockIdx.x * TILE + threadIdx.x;
    int u, v;
    float d;
    const bool keep = candidate(p, n, q, u, v, d) && kept(p, d);
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int i = 0; i < WAVES; ++i) s += wsum[i];
        p.ws[(size_t)n * p.nblk + blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(TILE) cloud_scan(int* ws, int* count, int nblk) {
    __shared__ int wtot[WAVES];
    int* w = ws + (size_t)blockIdx.x * nblk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;                                               // kept candidates in front of this chunk: the same value in every thread
    for (int b0 = 0; b0 < nblk; b0 += TILE) {
        const int b = b0 + threadIdx.x;
        const int c = b < nblk ? w[b] : 0;
        int inc = c;                                             // inclusive scan over the wave
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int o = __shfl_up(inc, s, 64);
            if (lane >= s) inc += o;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int base = carry, total = 0;
#pragma unroll
        for (int i = 0; i < WAVES; ++i) {
            if (i < wave) base += wtot[i];
            total += wtot[i];
        }
        if (b < nblk) w[b] = base + inc - c;                     // exclusive
        carry += total;
        __syncthreads();                                         // wtot is written again by the next chunk
    }
    if (threadIdx.x == 0) count[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(TILE) cloud_scatter(CloudP p) {
    __shared__ int wsum[WAVES];
    const int n = blockIdx.y, q = blockIdx.x * TILE + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int u = 0, v = 0;
    float d = 0.f;
    const bool keep = candidate(p, n, q, u, v, d) && kept(p, d);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    if (!keep) return;
    int at = p.ws[(size_t)n * p.nblk + blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int i = 0; i < wave; ++i) at += wsum[i];
    float x, y;
    pinhole_lift(pinhole_load(p.K + (size_t)n * 9), (float)u, (float)v, d, x, y);
    uint32_t rgba = 0xffffffffu;
    if (p.frame) {
        const uint8_t* f = p.frame + (((size_t)n * p.H + v) * p.W + u) * 3;
        rgba = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | 0xff000000u;
    }
    p.points[(size_t)n * p.cap + at] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(d), rgba);
}

// ---- dense mode ------------------------------------------------------------------------------------------------------------------------------
constexpr int NSUM = 12;           // dR row-major [3][3], then dt [3]

__global__ void __launch_bounds__(TILE) i2p_fwd(const float* __restrict__ depth, const float* __restrict__ R, const float* __restrict__ t, int t_pp,
                                                int H, int W, float* __restrict__ out) {
    const int b = blockIdx.y, npx = H * W, i = blockIdx.x * TILE + threadIdx.x;
    if (i >= npx) return;
    const int v = i / W, u = i - v * W;
    const float d = depth[(size_t)b * npx + i];
    const float g0 = (float)u * d, g1 = (float)v * d, g2 = d;
    const float* r = R + (size_t)b * 9;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float tc = t_pp ? t[((size_t)b * 3 + c) * npx + i] : t[b * 3 + c];
        out[((size_t)b * 3 + c) * npx + i] = r[3 * c] * g0 + r[3 * c + 1] * g1 + r[3 * c + 2] * g2 + tc;
    }
}

__global__ void __launch_bounds__(TILE) i2p_bwd(const float* __restrict__ g, const float* __restrict__ depth, const float* __restrict__ R, int H, int W,
                                                float* __restrict__ ddepth, float* __restrict__ part) {
    __shared__ float red[NSUM * WAVES];
    const int b = blockIdx.y, npx = H * W, i = blockIdx.x * TILE + threadIdx.x;
    float s[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) s[k] = 0.f;
    if (i < npx) {
        const int v = i / W, u = i - v * W;
        const float d = depth[(size_t)b * npx + i];
        const float* r = R + (size_t)b * 9;
        const float fu = (float)u, fv = (float)v;
        float dd = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gc = g[((size_t)b * 3 + c) * npx + i];
            dd += gc * (r[3 * c] * fu + r[3 * c + 1] * fv + r[3 * c + 2]);
            s[3 * c] = gc * (fu * d);
            s[3 * c + 1] = gc * (fv * d);
            s[3 * c + 2] = gc * d;
            s[9 + c] = gc;
        }
        ddepth[(size_t)b * npx + i] = dd;
    }
    if (!part) return;                                   // only ddepth was asked for (the same branch in every thread)
    sde_block_sums<NSUM, WAVES>(s, red, part + ((size_t)b * gridDim.x + blockIdx.x) * NSUM);
}

// one wave per sample: lane k < 12 adds sum k of every workgroup, in workgroup order, in fp64
__global__ void __launch_bounds__(64) i2p_bwd_finish(const float* __restrict__ part, int nblk, float* __restrict__ dR, float* __restrict__ dt) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= NSUM) return;
    const float* src = part + (size_t)b * nblk * NSUM + k;
    double acc = 0.0;
    for (int i = 0; i < nblk; ++i) acc += (double)src[(size_t)i * NSUM];
    if (k < 9) {
        if (dR) dR[b * 9 + k] = (float)acc;
    } else if (dt) dt[b * 3 + k - 9] = (float)acc;
}

bool cloud_shape_ok(int N, int H, int W, int step) {
    if (N <= 0 || H <= 0 || W <= 0 || step < 1 || N > 65535) return false;
    const long cap = (long)sde_cdiv(H, step) * sde_cdiv(W, step);
    return cap <= 0x7fffffffL - TILE && (long)N * sde_cdiv(cap, TILE) <= 0x7fffffffL / 4;
}

}  // namespace

extern "C" {

long sde_depth_cloud_capacity(int H, int W, int step) {
    if (!cloud_shape_ok(1, H, W, step)) return 0;
    return (long)sde_cdiv(H, step) * sde_cdiv(W, step);
}

size_t sde_depth_cloud_ws_bytes(int N, int H, int W, int step) {
    if (!cloud_shape_ok(N, H, W, step)) return 0;
    return (size_t)N * sde_cdiv(sde_depth_cloud_capacity(H, W, step), TILE) * sizeof(int);
}

int sde_depth_cloud(const float* pred, int N, int ph, int pw, const int* ymap, const int* xmap, int H, int W, const uint8_t* frame, const float* K,
                    float min_depth, float max_depth, int step, void* workspace, size_t workspace_bytes, void* points, int* count,
                    sde_stream_t stream) {
    SDE_CHECK_ARG(N > 0 && H > 0 && W > 0 && ph > 0 && pw > 0, "sde_depth_cloud: bad shape (N=%d, %dx%d -> %dx%d)", N, ph, pw, H, W);
    SDE_CHECK_ARG(step >= 1, "sde_depth_cloud: step must be at least 1 (%d)", step);
    SDE_CHECK_ARG(min_depth < max_depth, "sde_depth_cloud: min_depth must lie below max_depth (%g, %g)", (double)min_depth, (double)max_depth);
    SDE_CHECK_ARG(pred && ymap && xmap && K && points && count, "sde_depth_cloud: null pointer");
    SDE_CHECK_ARG(cloud_shape_ok(N, H, W, step) && (long)ph * pw <= 0x7fffffffL, "sde_depth_cloud: batch or map too large");
    SDE_CHECK_ARG(((uintptr_t)points & 15) == 0, "sde_depth_cloud: points must be 16-byte aligned");
    const size_t need = sde_depth_cloud_ws_bytes(N, H, W, step);
    SDE_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
                  "sde_depth_cloud: workspace of %zu bytes, sde_depth_cloud_ws_bytes asks for %zu", workspace ? workspace_bytes : (size_t)0, need);
    CloudP p{pred, ymap, xmap, frame, K, (int*)workspace, count, (uint4*)points, H, W, ph, pw, step, sde_cdiv(W, step), 0, 0, min_depth, max_depth};
    p.cap = (int)sde_depth_cloud_capacity(H, W, step);
    p.nblk = sde_cdiv(p.cap, TILE);
    const dim3 grid((unsigned)p.nblk, (unsigned)N);
    hipLaunchKernelGGL(cloud_count, grid, dim3(TILE), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(cloud_scan, dim3((unsigned)N), dim3(TILE), 0, (hipStream_t)stream, p.ws, count, p.nblk);
    hipLaunchKernelGGL(cloud_scatter, grid, dim3(TILE), 0, (hipStream_t)stream, p);
    SDE_CHECK_LAUNCH("sde_depth_cloud");
    return SDE_OK;
}

int sde_img_to_points_num_blocks(int H, int W) {
    if (H <= 0 || W <= 0 || (long)H * W > 0x7fffffffL - TILE) return 0;
    return sde_cdiv((long)H * W, TILE);
}

int sde_img_to_points_fwd(const float* depth, const float* R, const float* t, int t_per_pixel, int B, int H, int W, float* points,
                          sde_stream_t stream) {
    SDE_CHECK_ARG(B > 0 && B <= 65535 && sde_img_to_points_num_blocks(H, W) > 0, "sde_img_to_points_fwd: bad shape (B=%d, %dx%d)", B, H, W);
    SDE_CHECK_ARG(depth && R && t && points, "sde_img_to_points_fwd: null pointer");
    hipLaunchKernelGGL(i2p_fwd, dim3((unsigned)sde_img_to_points_num_blocks(H, W), (unsigned)B), dim3(TILE), 0, (hipStream_t)stream, depth, R, t,
                       t_per_pixel, H, W, points);
    SDE_CHECK_LAUNCH("sde_img_to_points_fwd");
    return SDE_OK;
}

int sde_img_to_points_bwd(const float* grad, const float* depth, const float* R, int B, int H, int W, float* part, float* ddepth, float* dR, float* dt,
                          sde_stream_t stream) {
    SDE_CHECK_ARG(B > 0 && B <= 65535 && sde_img_to_points_num_blocks(H, W) > 0, "sde_img_to_points_bwd: bad shape (B=%d, %dx%d)", B, H, W);
    SDE_CHECK_ARG(grad && depth && R && ddepth, "sde_img_to_points_bwd: null pointer");
    SDE_CHECK_ARG(part || (!dR && !dt), "sde_img_to_points_bwd: dR / dt need the partial-sum workspace");
    const int nblk = sde_img_to_points_num_blocks(H, W);
    const bool sums = dR || dt;
    hipLaunchKernelGGL(i2p_bwd, dim3((unsigned)nblk, (unsigned)B), dim3(TILE), 0, (hipStream_t)stream, grad, depth, R, H, W, ddepth, sums ? part : nullptr);
    if (sums) hipLaunchKernelGGL(i2p_bwd_finish, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, part, nblk, dR, dt);
    SDE_CHECK_LAUNCH("sde_img_to_points_bwd");
    return SDE_OK;
}

}  // extern "C"
