// The BTS decoder's own operators on gfx950 (reference: detectron2/modeling/depth_net/BTSNet.py:L39-275): everything around its
// convolutions that the engine in conv.hip does not already do.
//
//   dilate_split / dilate_merge  atrous convolution as space-to-batch (atrous_conv, L39-64): a 3x3 convolution with dilation d and
//                                pad d over [B,H,W,C] equals a 3x3, pad-1 convolution over the d*d phase images
//                                sub[(b*d + ph)*d + pw, i, j, :] = x[b, i*d + ph, j*d + pw, :] (zero beyond the map); merge is the inverse
//                                crop.  The GEMM in between is the ordinary conv engine (MFMA, all three passes); split and merge are each
//                                other's backward.  Taps that fall wholly outside the map are zero rows of the phase images.
//   upsample2                    F.interpolate(scale 2, nearest) of `upconv` (L67-79); backward sums the 2x2 blocks in fp32
//   cat                          torch.cat of up to SDE_CAT_MAX pieces with any channel counts (385 / 129 / 36 = ... + 1-channel fp32 maps)
//                                into one channel-padded NHWC tensor; backward splits the gradient back (fp32 maps stay planar fp32)
//   channel_stats                per-channel (sum, sum of squares) partial slab of a stored tensor: the batch statistics of `first_bn`, whose
//                                input is a concatenation no single GEMM epilogue produced
//   relu                         the nn.ReLU in front of daspp_3's first convolution
//   lpg                          reduction_1x1's plane head (sigmoid -> angles -> normal -> F.normalize, L110-122) fused with
//                                local_planar_guidance (L126-148), the / max_depth scaling and the nearest down-sampled copy (L238-240,L254-256)
//   sigmoid_head                 reduc1x1's final sigmoid and get_depth's sigmoid * max_depth (* focal / 715.0873), L183-188,L272-274
//
// All of it is bandwidth-bound: 16 bytes per lane on the NHWC tensors.  The plane head keeps the reference's operation order in fp32
// (this file is compiled without FMA contraction).
#include "vec16.h"
#include "launch.h"

namespace {

typedef SdeTypes<float, bf16_t, half_t> Types;
typedef SdeTypes<bf16_t, half_t, float> MoveTypes;      // the Bits<ES> kernels: the 2-byte instance comes first in the code object
constexpr int GRID_CAP = SDE_GRID_CAP_16K;

// ---------------------------------------------------------------------------------------------------------------------
// space-to-batch for dilated convolutions (pure data movement, raw bits)
// ---------------------------------------------------------------------------------------------------------------------
template <int ES, bool MERGE>
__global__ void __launch_bounds__(256) dilate_kernel(const void* __restrict__ in_, void* __restrict__ out_, int B, int H, int W, int C, int d, int Hs, int Ws) {
    const int V = Bits<ES>::V;
    const int cg = C / V;
    // MERGE: iterate over the [B,H,W] destination; split: over the [B*d*d, Hs, Ws] destination
    const long total = MERGE ? (long)B * H * W * cg : (long)B * d * d * Hs * Ws * cg;
    const uint4 z = {0u, 0u, 0u, 0u};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % cg);
        const long pix = i / cg;
        if (MERGE) {
            const int w = (int)(pix % W), h = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
            const long sb = ((long)b * d + h % d) * d + w % d;
            const long src = ((sb * Hs + h / d) * Ws + w / d) * C + (long)g * V;
            reinterpret_cast<uint4*>(out_)[pix * cg + g] = *reinterpret_cast<const uint4*>((const char*)in_ + src * ES);
        } else {
            const int j = (int)(pix % Ws), ii = (int)((pix / Ws) % Hs);
            const long sb = pix / ((long)Ws * Hs);
            const int pw = (int)(sb % d), ph = (int)((sb / d) % d), b = (int)(sb / ((long)d * d));
            const int h = ii * d + ph, w = j * d + pw;
            uint4 v = z;
            if (h < H && w < W) v = *reinterpret_cast<const uint4*>((const char*)in_ + ((((long)b * H + h) * W + w) * C + (long)g * V) * ES);
            reinterpret_cast<uint4*>(out_)[pix * cg + g] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// nearest x2 up-sampling and its backward (2x2 block sums)
// ---------------------------------------------------------------------------------------------------------------------
template <int ES>
__global__ void __launch_bounds__(256) up2_fwd_kernel(const void* __restrict__ in_, void* __restrict__ out_, int B, int H, int W, int C) {
    const int cg = C / Bits<ES>::V;
    const int OH = 2 * H, OW = 2 * W;
    const long total = (long)B * OH * OW * cg;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % cg);
        const long pix = i / cg;
        const int x = (int)(pix % OW), y = (int)((pix / OW) % OH), b = (int)(pix / ((long)OW * OH));
        const long src = (((long)b * H + (y >> 1)) * W + (x >> 1)) * cg + g;
        reinterpret_cast<uint4*>(out_)[i] = reinterpret_cast<const uint4*>(in_)[src];
    }
}

template <typename T>
__global__ void __launch_bounds__(256) up2_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dx, int B, int H, int W, int C) {
    constexpr int V = 16 / sizeof(T);
    const int cg = C / V;
    const long total = (long)B * H * W * cg;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % cg);
        const long pix = i / cg;
        const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = *reinterpret_cast<const uint4*>(dout + ((((long)b * 2 * H + 2 * y + (k >> 1)) * (2 * W) + 2 * x + (k & 1)) * C + (long)g * V));
            const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int q = 0; q < V; ++q) acc[q] += (float)e[q];
        }
        T o[V];
#pragma unroll
        for (int q = 0; q < V; ++q) o[q] = (T)acc[q];
        *reinterpret_cast<uint4*>(dx + pix * C + (long)g * V) = *reinterpret_cast<const uint4*>(o);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// multi-piece concatenation
// ---------------------------------------------------------------------------------------------------------------------
struct CatTable {
    sde_cat_piece p[SDE_CAT_MAX];
    int off[SDE_CAT_MAX + 1];     // first channel of every piece in the concatenated tensor; off[n] = channels used
    int n;
};

// fwd: one lane per (pixel, 16-byte group of the output)
template <typename T>
__global__ void __launch_bounds__(256) cat_fwd_kernel(const CatTable t, long P, int Ct, T* __restrict__ out) {
    constexpr int V = 16 / sizeof(T);
    const int cg = Ct / V;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P * cg; i += (long)gridDim.x * 256) {
        const int g = (int)(i % cg);
        const long pix = i / cg;
        const int c0 = g * V;
        int k = 0;
        while (k < t.n && t.off[k + 1] <= c0) ++k;
        T o[V];
        if (k < t.n && !t.p[k].f32map && t.off[k + 1] >= c0 + V && ((c0 - t.off[k]) % V) == 0) {
            // the whole group is 16 aligned bytes of one piece
            *reinterpret_cast<uint4*>(o) = *reinterpret_cast<const uint4*>((const T*)t.p[k].p + pix * t.p[k].ld + (c0 - t.off[k]));
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int c = c0 + e;
                while (k < t.n && t.off[k + 1] <= c) ++k;
                float v = 0.f;
                if (k < t.n) v = t.p[k].f32map ? ((const float*)t.p[k].p)[pix] : (float)((const T*)t.p[k].p)[pix * t.p[k].ld + (c - t.off[k])];
                o[e] = (T)v;
            }
        }
        *reinterpret_cast<uint4*>(out + pix * Ct + c0) = *reinterpret_cast<const uint4*>(o);
    }
}

// bwd: one lane per (pixel, destination group) -- groups of all pieces laid end to end (a planar fp32 map counts one group)
template <typename T>
__global__ void __launch_bounds__(256) cat_bwd_kernel(const CatTable t, long P, int Ct, const T* __restrict__ dout, int gtot) {
    constexpr int V = 16 / sizeof(T);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P * gtot; i += (long)gridDim.x * 256) {
        int g = (int)(i % gtot);
        const long pix = i / gtot;
        int k = 0;
        for (; k < t.n; ++k) {
            const int gk = t.p[k].f32map ? 1 : t.p[k].ld / V;
            if (g < gk) break;
            g -= gk;
        }
        const sde_cat_piece& pc = t.p[k];
        const T* src = dout + pix * Ct + t.off[k];
        if (pc.f32map) { ((float*)pc.p)[pix] = (float)src[0]; continue; }
        const int c0 = g * V;
        T* dst = (T*)pc.p + pix * pc.ld + c0;
        if (c0 + V <= pc.C && (t.off[k] % V) == 0) {
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src + c0);
        } else {
            T o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = (c0 + e < pc.C) ? src[c0 + e] : (T)0.f;
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(o);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// per-channel (sum, sum of squares) partials: part[tile][c][2], a tile = SDE_STATS_ROWS rows; fixed order, no atomics
// ---------------------------------------------------------------------------------------------------------------------
constexpr int STATS_GROUPS = 32;      // 16-byte channel groups per workgroup
constexpr int STATS_LANES = 8;        // row lanes per workgroup

template <typename T>
__global__ void __launch_bounds__(256) channel_stats_kernel(const T* __restrict__ x, long M, int C, float* __restrict__ part) {
    constexpr int V = 16 / sizeof(T);
    __shared__ float red[STATS_LANES][STATS_GROUPS * V * 2];
    const int tile = blockIdx.x, gl = threadIdx.x % STATS_GROUPS, rl = threadIdx.x / STATS_GROUPS;
    const int g = blockIdx.y * STATS_GROUPS + gl;
    const int cg = C / V;
    float s1[V], s2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
    if (g < cg) {
        const long r1 = min(M, (long)(tile + 1) * SDE_STATS_ROWS);
        for (long r = (long)tile * SDE_STATS_ROWS + rl; r < r1; r += STATS_LANES) {
            const uint4 v = *reinterpret_cast<const uint4*>(x + r * C + (long)g * V);
            const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int q = 0; q < V; ++q) { const float f = (float)e[q]; s1[q] += f; s2[q] += f * f; }
        }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) { red[rl][(gl * V + q) * 2] = s1[q]; red[rl][(gl * V + q) * 2 + 1] = s2[q]; }
    __syncthreads();
    for (int j = threadIdx.x; j < STATS_GROUPS * V * 2; j += 256) {
        const int c = blockIdx.y * STATS_GROUPS * V + j / 2;
        if (c >= C) continue;
        float a = 0.f;
#pragma unroll
        for (int l = 0; l < STATS_LANES; ++l) a += red[l][j];
        part[((long)tile * C + c) * 2 + (j & 1)] = a;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) relu_kernel(const T* __restrict__ x, T* __restrict__ y, long n) {
    constexpr int V = 16 / sizeof(T);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n / V; i += (long)gridDim.x * 256) {
        const uint4 v = reinterpret_cast<const uint4*>(x)[i];
        const T* e = reinterpret_cast<const T*>(&v);
        T o[V];
#pragma unroll
        for (int q = 0; q < V; ++q) o[q] = (float)e[q] > 0.f ? e[q] : (T)0.f;
        reinterpret_cast<uint4*>(y)[i] = *reinterpret_cast<const uint4*>(o);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// plane head + local planar guidance
// ---------------------------------------------------------------------------------------------------------------------
struct Plane { float s0, s1, s2, st, ct, sp, cp, m1, m2, m3, nrm, n1, n2, n3, n4; };

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// reduction_1x1.forward (L110-122) and the F.normalize of bts.forward (L235-236), in the reference's operation order
__device__ __forceinline__ Plane plane_of(float a0, float a1, float a2, float max_depth) {
    Plane p;
    p.s0 = sigm(a0); p.s1 = sigm(a1); p.s2 = sigm(a2);
    const float theta = p.s0 * 3.14159265358979323846f / 3.f;
    const float phi = p.s1 * 3.14159265358979323846f * 2.f;
    p.n4 = p.s2 * max_depth;
    p.st = sinf(theta); p.ct = cosf(theta); p.sp = sinf(phi); p.cp = cosf(phi);
    p.m1 = p.st * p.cp; p.m2 = p.st * p.sp; p.m3 = p.ct;
    p.nrm = sqrtf(p.m1 * p.m1 + p.m2 * p.m2 + p.m3 * p.m3);
    const float dn = fmaxf(p.nrm, 1e-12f);
    p.n1 = p.m1 / dn; p.n2 = p.m2 / dn; p.n3 = p.m3 / dn;
    return p;
}

__device__ __forceinline__ float lpg_coord(int k, int r) { return ((float)k - (float)(r - 1) * 0.5f) / (float)r; }

template <typename T>
__global__ void __launch_bounds__(256) lpg_fwd_kernel(const T* __restrict__ y, int B, int h, int w, int ld, int r, float max_depth, int ds, float* __restrict__ full,
                                                      float* __restrict__ down) {
    const int H = h * r, W = w * r;
    const long total = (long)B * H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int J = (int)(i % W), I = (int)((i / W) % H), b = (int)(i / ((long)W * H));
        const T* a = y + (((long)b * h + I / r) * w + J / r) * ld;
        const Plane p = plane_of((float)a[0], (float)a[1], (float)a[2], max_depth);
        const float u = lpg_coord(J % r, r), v = lpg_coord(I % r, r);
        const float den = p.n1 * u + p.n2 * v + p.n3;
        const float d = (p.n4 / den) / max_depth;
        full[i] = d;
        if (ds > 0 && (I % ds) == 0 && (J % ds) == 0) down[((long)b * (H / ds) + I / ds) * (W / ds) + J / ds] = d;
    }
}

// one lane per plane: sums the r x r pixels' gradients (both consumers), then back through normalize, the angles and the sigmoids
template <typename T>
__global__ void __launch_bounds__(256) lpg_bwd_kernel(const T* __restrict__ y, const float* __restrict__ dfull, const float* __restrict__ ddown, int B, int h, int w,
                                                      int ld, int r, float max_depth, int ds, T* __restrict__ dy) {
    const int H = h * r, W = w * r;
    const long total = (long)B * h * w;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int j = (int)(i % w), ii = (int)((i / w) % h), b = (int)(i / ((long)w * h));
        const T* a = y + i * ld;
        const Plane p = plane_of((float)a[0], (float)a[1], (float)a[2], max_depth);
        float g1 = 0.f, g2 = 0.f, g3 = 0.f, g4 = 0.f;
        for (int dv = 0; dv < r; ++dv) {
            const int I = ii * r + dv;
            const float v = lpg_coord(dv, r);
            for (int du = 0; du < r; ++du) {
                const int J = j * r + du;
                float g = dfull ? dfull[((long)b * H + I) * W + J] : 0.f;
                if (ddown && ds > 0 && (I % ds) == 0 && (J % ds) == 0) g += ddown[((long)b * (H / ds) + I / ds) * (W / ds) + J / ds];
                const float u = lpg_coord(du, r);
                const float den = p.n1 * u + p.n2 * v + p.n3;
                const float gd = g / max_depth;                    // d loss / d (n4 / den)
                g4 += gd / den;
                const float gden = -gd * p.n4 / (den * den);
                g1 += gden * u; g2 += gden * v; g3 += gden;
            }
        }
        // F.normalize: n = m / max(|m|, eps)
        float dm1, dm2, dm3;
        if (p.nrm > 1e-12f) {
            const float dot = p.n1 * g1 + p.n2 * g2 + p.n3 * g3;
            dm1 = (g1 - p.n1 * dot) / p.nrm; dm2 = (g2 - p.n2 * dot) / p.nrm; dm3 = (g3 - p.n3 * dot) / p.nrm;
        } else {
            dm1 = g1 / 1e-12f; dm2 = g2 / 1e-12f; dm3 = g3 / 1e-12f;
        }
        const float dtheta = dm1 * p.ct * p.cp + dm2 * p.ct * p.sp - dm3 * p.st;
        const float dphi = -dm1 * p.st * p.sp + dm2 * p.st * p.cp;
        const float da0 = dtheta * (3.14159265358979323846f / 3.f) * p.s0 * (1.f - p.s0);
        const float da1 = dphi * (3.14159265358979323846f * 2.f) * p.s1 * (1.f - p.s1);
        const float da2 = g4 * max_depth * p.s2 * (1.f - p.s2);
        T* o = dy + i * ld;
        for (int c = 0; c < ld; ++c) o[c] = (T)(c == 0 ? da0 : c == 1 ? da1 : c == 2 ? da2 : 0.f);
    }
}

// out[b,0,h,x] = sigmoid(y[b,h,x',0]) * scale [* focal[b] / focal_div], x' = x or W-1-x (flip)
template <typename T>
__global__ void __launch_bounds__(256) sigmoid_head_fwd_kernel(const T* __restrict__ y, int B, int H, int W, int ld, float scale, const float* __restrict__ focal,
                                                               float focal_div, int flip, float* __restrict__ out) {
    const long total = (long)B * H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % W);
        const long row = i / W;
        const int b = (int)(row / H);
        const int xs = flip ? W - 1 - x : x;
        float v = sigm((float)y[(row * W + xs) * ld]) * scale;
        if (focal) v = (v * focal[b]) / focal_div;
        out[i] = v;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) sigmoid_head_bwd_kernel(const T* __restrict__ y, const float* __restrict__ dout, int B, int H, int W, int ld, float scale,
                                                               const float* __restrict__ focal, float focal_div, int flip, T* __restrict__ dy) {
    const long total = (long)B * H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % W);
        const long row = i / W;
        const int b = (int)(row / H);
        const int xs = flip ? W - 1 - x : x;
        T* o = dy + (row * W + xs) * ld;
        const float s = sigm((float)y[(row * W + xs) * ld]);
        float g = dout[i];
        if (focal) g = (g / focal_div) * focal[b];
        g = g * scale * s * (1.f - s);
        o[0] = (T)g;
        for (int c = 1; c < ld; ++c) o[c] = (T)0.f;
    }
}

}  // namespace

extern "C" {

int sde_dilate_split(const void* x, int B, int H, int W, int C, int d, int dtype, void* out, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(x && out && Types::has(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % V == 0 && d >= 1, "sde_dilate_split: bad argument (dtype %d)", dtype);
    const int Hs = (H + d - 1) / d, Ws = (W + d - 1) / d;
    const int nb = sde_grid_for((long)B * d * d * Hs * Ws * (C / V), GRID_CAP);
    MoveTypes::dispatch(dtype, [&](auto tag) {
        hipLaunchKernelGGL((dilate_kernel<decltype(tag)::size, false>), dim3(nb), dim3(256), 0, (hipStream_t)stream, x, out, B, H, W, C, d, Hs, Ws);
    });
    SDE_CHECK_LAUNCH("sde_dilate_split");
    return SDE_OK;
}

int sde_dilate_merge(const void* sub, int B, int H, int W, int C, int d, int dtype, void* out, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(sub && out && Types::has(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % V == 0 && d >= 1, "sde_dilate_merge: bad argument (dtype %d)", dtype);
    const int Hs = (H + d - 1) / d, Ws = (W + d - 1) / d;
    const int nb = sde_grid_for((long)B * H * W * (C / V), GRID_CAP);
    MoveTypes::dispatch(dtype, [&](auto tag) {
        hipLaunchKernelGGL((dilate_kernel<decltype(tag)::size, true>), dim3(nb), dim3(256), 0, (hipStream_t)stream, sub, out, B, H, W, C, d, Hs, Ws);
    });
    SDE_CHECK_LAUNCH("sde_dilate_merge");
    return SDE_OK;
}

int sde_upsample2_fwd(const void* x, int B, int H, int W, int C, int dtype, void* out, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(x && out && Types::has(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % V == 0, "sde_upsample2_fwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for((long)B * 4 * H * W * (C / V), GRID_CAP);
    MoveTypes::dispatch(dtype, [&](auto tag) {
        hipLaunchKernelGGL(up2_fwd_kernel<decltype(tag)::size>, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, out, B, H, W, C);
    });
    SDE_CHECK_LAUNCH("sde_upsample2_fwd");
    return SDE_OK;
}

int sde_upsample2_bwd(const void* dout, int B, int H, int W, int C, int dtype, void* dx, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(dout && dx && Types::has(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % V == 0, "sde_upsample2_bwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for((long)B * H * W * (C / V), GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(up2_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)dout, (T*)dx, B, H, W, C);
    });
    SDE_CHECK_LAUNCH("sde_upsample2_bwd");
    return SDE_OK;
}

static int cat_table(const sde_cat_piece* pieces, int n, int Ct, int V, CatTable& t, const char* who) {
    SDE_CHECK_ARG(pieces && n >= 1 && n <= SDE_CAT_MAX && Ct > 0 && Ct % V == 0, "%s: bad piece list (n=%d, Ct=%d)", who, n, Ct);
    t.n = n;
    t.off[0] = 0;
    for (int k = 0; k < n; ++k) {
        const sde_cat_piece& p = pieces[k];
        SDE_CHECK_ARG(p.p && p.C > 0 && (p.f32map ? (p.C == 1) : (p.ld >= p.C && p.ld % V == 0)), "%s: bad piece %d (C=%d ld=%d)", who, k, p.C, p.ld);
        t.p[k] = p;
        t.off[k + 1] = t.off[k] + p.C;
    }
    for (int k = n; k < SDE_CAT_MAX; ++k) { t.p[k] = sde_cat_piece{}; t.off[k + 1] = t.off[n]; }
    SDE_CHECK_ARG(t.off[n] <= Ct && Ct < t.off[n] + V, "%s: %d channels do not pad to %d", who, t.off[n], Ct);
    return SDE_OK;
}

int sde_cat_fwd(const sde_cat_piece* pieces, int n, long P, int Ct, int dtype, void* out, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(out && Types::has(dtype) && P > 0, "sde_cat_fwd: bad argument (dtype %d)", dtype);
    CatTable t;
    const int rc = cat_table(pieces, n, Ct, V, t, "sde_cat_fwd");
    if (rc) return rc;
    const int nb = sde_grid_for(P * (Ct / V), GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(cat_fwd_kernel<T>, dim3(nb), dim3(256), 0, s, t, P, Ct, (T*)out);
    });
    SDE_CHECK_LAUNCH("sde_cat_fwd");
    return SDE_OK;
}

int sde_cat_bwd(const void* dout, long P, int Ct, int dtype, const sde_cat_piece* grads, int n, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(dout && Types::has(dtype) && P > 0, "sde_cat_bwd: bad argument (dtype %d)", dtype);
    CatTable t;
    const int rc = cat_table(grads, n, Ct, V, t, "sde_cat_bwd");
    if (rc) return rc;
    int gtot = 0;
    for (int k = 0; k < n; ++k) gtot += grads[k].f32map ? 1 : grads[k].ld / V;
    const int nb = sde_grid_for(P * gtot, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(cat_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, t, P, Ct, (const T*)dout, gtot);
    });
    SDE_CHECK_LAUNCH("sde_cat_bwd");
    return SDE_OK;
}

int sde_channel_stats_tiles(long M) { return M > 0 ? sde_cdiv(M, SDE_STATS_ROWS) : 0; }

int sde_channel_stats(const void* x, long M, int C, int dtype, float* part, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(x && part && Types::has(dtype) && M > 0 && C > 0 && C % V == 0, "sde_channel_stats: bad argument (dtype %d)", dtype);
    const dim3 grid(sde_channel_stats_tiles(M), sde_cdiv(C / V, STATS_GROUPS));
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(channel_stats_kernel<T>, grid, dim3(256), 0, s, (const T*)x, M, C, part);
    });
    SDE_CHECK_LAUNCH("sde_channel_stats");
    return SDE_OK;
}

int sde_relu_fwd(const void* x, long n, int dtype, void* y, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(x && y && Types::has(dtype) && n > 0 && n % V == 0, "sde_relu_fwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for(n / V, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(relu_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)x, (T*)y, n);
    });
    SDE_CHECK_LAUNCH("sde_relu_fwd");
    return SDE_OK;
}

int sde_lpg_fwd(const void* y, int B, int h, int w, int ld, int r, float max_depth, int ds, int dtype, float* full, float* down, sde_stream_t stream) {
    SDE_CHECK_ARG(y && full && Types::has(dtype) && B > 0 && h > 0 && w > 0 && ld >= 3 && r >= 1 && max_depth > 0.f, "sde_lpg_fwd: bad argument (dtype %d)", dtype);
    SDE_CHECK_ARG(ds == 0 || (down && (h * r) % ds == 0 && (w * r) % ds == 0), "sde_lpg_fwd: bad down-sampling (%d)", ds);
    const int nb = sde_grid_for((long)B * h * r * w * r, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(lpg_fwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)y, B, h, w, ld, r, max_depth, ds, full, down);
    });
    SDE_CHECK_LAUNCH("sde_lpg_fwd");
    return SDE_OK;
}

int sde_lpg_bwd(const void* y, const float* dfull, const float* ddown, int B, int h, int w, int ld, int r, float max_depth, int ds, int dtype, void* dy,
                sde_stream_t stream) {
    SDE_CHECK_ARG(y && dy && Types::has(dtype) && B > 0 && h > 0 && w > 0 && ld >= 3 && r >= 1 && max_depth > 0.f, "sde_lpg_bwd: bad argument (dtype %d)", dtype);
    SDE_CHECK_ARG(!ddown || (ds > 0 && (h * r) % ds == 0 && (w * r) % ds == 0), "sde_lpg_bwd: bad down-sampling (%d)", ds);
    const int nb = sde_grid_for((long)B * h * w, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(lpg_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)y, dfull, ddown, B, h, w, ld, r, max_depth, ds, (T*)dy);
    });
    SDE_CHECK_LAUNCH("sde_lpg_bwd");
    return SDE_OK;
}

int sde_sigmoid_head_fwd(const void* y, int B, int H, int W, int ld, float scale, const float* focal, float focal_div, int flip, int dtype, float* out,
                         sde_stream_t stream) {
    SDE_CHECK_ARG(y && out && Types::has(dtype) && B > 0 && H > 0 && W > 0 && ld >= 1 && (!focal || focal_div != 0.f), "sde_sigmoid_head_fwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for((long)B * H * W, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(sigmoid_head_fwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)y, B, H, W, ld, scale, focal, focal_div, flip, out);
    });
    SDE_CHECK_LAUNCH("sde_sigmoid_head_fwd");
    return SDE_OK;
}

int sde_sigmoid_head_bwd(const void* y, const float* dout, int B, int H, int W, int ld, float scale, const float* focal, float focal_div, int flip, int dtype,
                         void* dy, sde_stream_t stream) {
    SDE_CHECK_ARG(y && dout && dy && Types::has(dtype) && B > 0 && H > 0 && W > 0 && ld >= 1 && (!focal || focal_div != 0.f), "sde_sigmoid_head_bwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for((long)B * H * W, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(sigmoid_head_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)y, dout, B, H, W, ld, scale, focal, focal_div, flip, (T*)dy);
    });
    SDE_CHECK_LAUNCH("sde_sigmoid_head_bwd");
    return SDE_OK;
}

}  // extern "C"
