// GoogleMotionNet / GooglePoseNet operators on gfx950 (reference: detectron2/modeling/pose_net/GooglePoseNet.py): what surrounds the convolutions
// of the motion refiners and is not already in conv.hip / nn.hip / google.hip.
//
//   resize_cat   MotionRefiner (L91-94): F.interpolate(field, size=skip's, mode='bilinear', align_corners=True) and cat([field, skip], 1) in
//                one pass.  The 3-channel field is fp32 [B,h,w,4] (the trunk is summed over eight refiners and stays fp32 in both modes); the
//                result X [B,H,W,Cx] is in the compute dtype, channels [field(3), skip(Cr), zeros] -- the reference's order, so conv weights
//                need no permutation -- and the resized field is also kept as fp32 `up` [B,H,W,4] for the residual add of the tail.
//                Backward: every field pixel gathers the output taps that read it (any ratio, 1-pixel maps included); the skip's gradient is
//                written dense by the same launch; up to two gradients of X (its two consumers) plus the one of `up` are summed on the fly.
//   tail         out = up + conv3(cat[out1, out2]) (L95-99), conv3 a bias-free 1x1 to 3 channels: pointwise, reads out1 and out2 directly.
//                Backward: d out1 / d out2, and the weight gradient as per-workgroup partials [blocks][3][2 mid] + a fixed-order final sum.
//   head         motion_pred = field * scale [* (|field * scale| > mean)] * weight as planar fp32 NCHW (L190-205); scale and weight are
//                read from device memory.  [sum] per-workgroup partial sums of the norm, [apply] fp64 mean from the partials, mask, store.
//                Backward: d field and per-workgroup partials of d scale.
//   prep_bwd     the gradient of sde_prep_input without mean / std / flip: NHWC compute dtype -> planar fp32 NCHW, two gradients summed.
//
// No atomics anywhere: every sum has one owner and a fixed order, so repeated runs give identical bits.
#include "vec16.h"
#include "launch.h"

namespace {

typedef SdeTypes<float, bf16_t> Types;
constexpr int GRID_CAP = SDE_GRID_CAP_16K;

// ---------------------------------------------------------------------------------------------------------------------
// resize (align_corners=True, any ratio) + cat
// ---------------------------------------------------------------------------------------------------------------------
struct Tap {
    int i0, i1;
    float l0, l1;
};

// torch's area_pixel_compute_scale for align_corners=True
__host__ __device__ __forceinline__ float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

__device__ __forceinline__ Tap tap(int o, int in, float scale) {
    const float src = scale * (float)o;
    Tap t;
    t.i0 = min((int)src, in - 1);
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
    t.l0 = 1.f - t.l1;
    return t;
}

template <typename T>
__global__ void __launch_bounds__(256) resize_cat_fwd_kernel(const float* __restrict__ field, int h, int w, const T* __restrict__ skip, int B, int H, int W,
                                                             int Cs, int Cr, int Cx, T* __restrict__ X, float* __restrict__ up) {
    constexpr int V = VecOf<T>::V;
    const int cch = Cx / V;
    const float sh = ac_scale(h, H), sw = ac_scale(w, W);
    const long total = (long)B * H * W * cch;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % cch);
        const long pix = i / cch;
        float o[V];
        const T* sp = skip + pix * Cs;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int c = g * V + e - 3;
            o[e] = (c >= 0 && c < Cr) ? (float)sp[c] : 0.f;
        }
        if (g == 0) {
            const int ox = (int)(pix % W), oy = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
            const Tap ty = tap(oy, h, sh), tx = tap(ox, w, sw);
            const float* fb = field + (long)b * h * w * 4;
            const float4 v00 = *reinterpret_cast<const float4*>(fb + ((long)ty.i0 * w + tx.i0) * 4);
            const float4 v01 = *reinterpret_cast<const float4*>(fb + ((long)ty.i0 * w + tx.i1) * 4);
            const float4 v10 = *reinterpret_cast<const float4*>(fb + ((long)ty.i1 * w + tx.i0) * 4);
            const float4 v11 = *reinterpret_cast<const float4*>(fb + ((long)ty.i1 * w + tx.i1) * 4);
            o[0] = ty.l0 * (tx.l0 * v00.x + tx.l1 * v01.x) + ty.l1 * (tx.l0 * v10.x + tx.l1 * v11.x);
            o[1] = ty.l0 * (tx.l0 * v00.y + tx.l1 * v01.y) + ty.l1 * (tx.l0 * v10.y + tx.l1 * v11.y);
            o[2] = ty.l0 * (tx.l0 * v00.z + tx.l1 * v01.z) + ty.l1 * (tx.l0 * v10.z + tx.l1 * v11.z);
            *reinterpret_cast<float4*>(up + pix * 4) = make_float4(o[0], o[1], o[2], 0.f);
        }
        store_vec<T>(X + i * V, o);
    }
}

// Output positions along one axis that may read input index i: a conservative range, the exact test is the forward's own tap().
__device__ __forceinline__ void gather_range(int i, int in, int out, float scale, int* lo, int* hi) {
    if (scale <= 0.f) { *lo = 0; *hi = out - 1; return; }
    const float inv = 1.f / scale;
    *lo = max(0, (int)floorf((float)(i - 1) * inv) - 1);
    *hi = min(out - 1, (int)ceilf((float)(i + 1) * inv) + 1);
}

template <typename T>
__global__ void __launch_bounds__(256) resize_cat_bwd_kernel(const T* __restrict__ d0, const T* __restrict__ d1, const float* __restrict__ dup, int B, int H,
                                                             int W, int Cx, int Cr, int Cs, int h, int w, float* __restrict__ dfield,
                                                             T* __restrict__ dskip) {
    constexpr int V = VecOf<T>::V;
    // 1. the skip's gradient: channels 3 .. 3 + Cr of the summed gradient, dense with zero pad channels
    if (dskip) {
        const int cch = Cs / V;
        const long total = (long)B * H * W * cch;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const int g = (int)(i % cch);
            const long pix = i / cch;
            // channels 3 + gV .. 3 + gV + V of X straddle its 16-byte groups g and g + 1 (Cx >= Cr + 3: group g + 1 exists wherever it is needed)
            float two[2 * V], o[V];
#pragma unroll
            for (int e = 0; e < 2 * V; ++e) two[e] = 0.f;
            const bool first = g * V < Cx, second = (g + 1) * V < Cx;      // Cs may exceed Cx: such groups hold no real channel
            for (int k = 0; k < 2; ++k) {
                const T* d = k ? d1 : d0;
                if (!d || !first) continue;
                float v[V];
                load_vec<T>(d + pix * Cx + g * V, v);
#pragma unroll
                for (int e = 0; e < V; ++e) two[e] += v[e];
                if (second) {
                    load_vec<T>(d + pix * Cx + (g + 1) * V, v);
#pragma unroll
                    for (int e = 0; e < V; ++e) two[V + e] += v[e];
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = (g * V + e < Cr) ? two[3 + e] : 0.f;
            store_vec<T>(dskip + i * V, o);
        }
    }
    // 2. the field's gradient: gather form
    const float sh = ac_scale(h, H), sw = ac_scale(w, W);
    const long total = (long)B * h * w;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ix = (int)(i % w), iy = (int)((i / w) % h), b = (int)(i / ((long)w * h));
        int ylo, yhi, xlo, xhi;
        gather_range(iy, h, H, sh, &ylo, &yhi);
        gather_range(ix, w, W, sw, &xlo, &xhi);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int oy = ylo; oy <= yhi; ++oy) {
            const Tap ty = tap(oy, h, sh);
            const float wy = (ty.i0 == iy ? ty.l0 : 0.f) + (ty.i1 == iy ? ty.l1 : 0.f);
            if (ty.i0 != iy && ty.i1 != iy) continue;
            for (int ox = xlo; ox <= xhi; ++ox) {
                const Tap tx = tap(ox, w, sw);
                if (tx.i0 != ix && tx.i1 != ix) continue;
                const float wt = wy * ((tx.i0 == ix ? tx.l0 : 0.f) + (tx.i1 == ix ? tx.l1 : 0.f));
                const long pix = ((long)b * H + oy) * W + ox;
                float g0 = 0.f, g1 = 0.f, g2 = 0.f;
                if (d0) { const T* p = d0 + pix * Cx; g0 += (float)p[0]; g1 += (float)p[1]; g2 += (float)p[2]; }
                if (d1) { const T* p = d1 + pix * Cx; g0 += (float)p[0]; g1 += (float)p[1]; g2 += (float)p[2]; }
                if (dup) { const float4 u = *reinterpret_cast<const float4*>(dup + pix * 4); g0 += u.x; g1 += u.y; g2 += u.z; }
                a0 += wt * g0; a1 += wt * g1; a2 += wt * g2;
            }
        }
        *reinterpret_cast<float4*>(dfield + i * 4) = make_float4(a0, a1, a2, 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// refiner tail: out = up + W3 . cat[o1, o2]
// ---------------------------------------------------------------------------------------------------------------------
// Lanes that share one pixel: a power of two <= 64 and <= the 16-byte channel groups of cat[o1, o2].
int tail_tpp(int groups2) {
    int t = 1;
    while (t * 2 <= groups2 && t < 64) t *= 2;
    return t;
}

template <typename T>
__global__ void __launch_bounds__(256) tail_fwd_kernel(const T* __restrict__ o1, const T* __restrict__ o2, const float* __restrict__ w3,
                                                       const float* __restrict__ up, long P, int ld, int mid, int tpp, float* __restrict__ out) {
    constexpr int V = VecOf<T>::V;
    const int groups = ld / V, groups2 = 2 * groups;
    const int ppb = 256 / tpp;                     // pixels per workgroup and sweep
    const int sub = threadIdx.x % tpp, slot = threadIdx.x / tpp;
    for (long base = (long)blockIdx.x * ppb; base < P; base += (long)gridDim.x * ppb) {      // uniform trip count: the shuffles below need every lane
        const long pix = base + slot;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (pix < P) {
            for (int g2 = sub; g2 < groups2; g2 += tpp) {
                const int half = g2 >= groups, g = half ? g2 - groups : g2;
                float v[V];
                load_vec<T>((half ? o2 : o1) + pix * ld + g * V, v);
                const int c0 = g * V;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    if (c0 + e < mid) {
                        const int k = half * mid + c0 + e;
                        a0 += v[e] * w3[k];
                        a1 += v[e] * w3[2 * mid + k];
                        a2 += v[e] * w3[4 * mid + k];
                    }
                }
            }
        }
        for (int off = tpp >> 1; off > 0; off >>= 1) {
            a0 += __shfl_xor(a0, off, 64);
            a1 += __shfl_xor(a1, off, 64);
            a2 += __shfl_xor(a2, off, 64);
        }
        if (sub == 0 && pix < P) {
            const float4 u = *reinterpret_cast<const float4*>(up + pix * 4);
            *reinterpret_cast<float4*>(out + pix * 4) = make_float4(u.x + a0, u.y + a1, u.z + a2, 0.f);
        }
    }
}

constexpr int TAIL_MAX_BLOCKS = 1024;

// Workgroup layout of the backward: CH lanes over the channel groups of cat[o1, o2], 256 / CH pixel slots.
int tail_bwd_ch(int groups2) { return groups2 < 256 ? groups2 : 256; }
int tail_bwd_blocks(long P, int groups2) {
    const int slots = 256 / tail_bwd_ch(groups2);
    long nb = (P + slots - 1) / slots;
    if (nb > TAIL_MAX_BLOCKS) nb = TAIL_MAX_BLOCKS;
    return (int)(nb < 1 ? 1 : nb);
}

template <typename T>
__global__ void __launch_bounds__(256) tail_bwd_kernel(const float* __restrict__ dout, const T* __restrict__ o1, const T* __restrict__ o2,
                                                       const float* __restrict__ w3, long P, int ld, int mid, int CH, T* __restrict__ do1,
                                                       T* __restrict__ do2, float* __restrict__ part) {
    constexpr int V = VecOf<T>::V;
    __shared__ float red[256 * 3 * V];
    const int groups = ld / V, groups2 = 2 * groups;
    const int slots = 256 / CH;
    const int cl = threadIdx.x % CH, slot = threadIdx.x / CH;
    const bool lane_ok = slot < slots;
    for (int gbase = 0; gbase < groups2; gbase += CH) {                                   // uniform: __syncthreads inside
        const int g2 = gbase + cl;
        const bool active = lane_ok && g2 < groups2;
        const int half = g2 >= groups, g = half ? g2 - groups : g2;
        const int c0 = g * V;
        float wv[3][V], acc[3][V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const bool real = active && c0 + e < mid;
            const int k = half * mid + c0 + e;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                wv[j][e] = real ? w3[2 * j * mid + k] : 0.f;
                acc[j][e] = 0.f;
            }
        }
        if (active) {
            const T* src = half ? o2 : o1;
            T* dst = half ? do2 : do1;
            for (long pix = (long)blockIdx.x * slots + slot; pix < P; pix += (long)gridDim.x * slots) {
                const float4 d = *reinterpret_cast<const float4*>(dout + pix * 4);
                float v[V], o[V];
                load_vec<T>(src + pix * ld + c0, v);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    o[e] = d.x * wv[0][e] + d.y * wv[1][e] + d.z * wv[2][e];
                    acc[0][e] += d.x * v[e];
                    acc[1][e] += d.y * v[e];
                    acc[2][e] += d.z * v[e];
                }
                store_vec<T>(dst + pix * ld + c0, o);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int e = 0; e < V; ++e) red[(threadIdx.x * 3 + j) * V + e] = acc[j][e];
        __syncthreads();
        // fixed-order tree over the pixel slots: slot q takes slot q + stride
        int top = 1;
        while (top < slots) top <<= 1;
        for (int stride = top >> 1; stride > 0; stride >>= 1) {
            if (lane_ok && slot < stride && slot + stride < slots) {
#pragma unroll
                for (int k = 0; k < 3 * V; ++k) red[threadIdx.x * 3 * V + k] += red[(threadIdx.x + stride * CH) * 3 * V + k];
            }
            __syncthreads();
        }
        if (active && slot == 0) {
            for (int j = 0; j < 3; ++j)
                for (int e = 0; e < V; ++e)
                    if (c0 + e < mid) part[((long)blockIdx.x * 3 + j) * 2 * mid + half * mid + c0 + e] = red[(cl * 3 + j) * V + e];
        }
    }
}

// 4 outputs per workgroup, 64 row lanes each: fp64 partial sums, then a fixed-order tree
__global__ void __launch_bounds__(256) tail_bwd_final_kernel(const float* __restrict__ part, int nblk, int n, float* __restrict__ dw3) {
    __shared__ double red[256];
    const int c = threadIdx.x & 3, r = threadIdx.x >> 2;
    const int i = blockIdx.x * 4 + c;
    double s = 0.0;
    if (i < n)
        for (int b = r; b < nblk; b += 64) s += (double)part[(long)b * n + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (r < off) red[threadIdx.x] += red[threadIdx.x + off * 4];
        __syncthreads();
    }
    if (r == 0 && i < n) dw3[i] = (float)red[c];
}

// ---------------------------------------------------------------------------------------------------------------------
// scale + mask + weight head
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HEAD_MAX_BLOCKS = 1024;

int head_blocks(long P) {
    long nb = (P + 255) / 256;
    if (nb > HEAD_MAX_BLOCKS) nb = HEAD_MAX_BLOCKS;
    return (int)(nb < 1 ? 1 : nb);
}

// |field * scale| with a fixed operation order (no FMA contraction), so both launches of the forward get the same bits
__device__ __forceinline__ float scaled_norm(float4 m, float s, float* r) {
    r[0] = __fmul_rn(m.x, s); r[1] = __fmul_rn(m.y, s); r[2] = __fmul_rn(m.z, s);
    return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(r[0], r[0]), __fmul_rn(r[1], r[1])), __fmul_rn(r[2], r[2])));
}

__global__ void __launch_bounds__(256) head_sum_kernel(const float* __restrict__ m, const float* __restrict__ scale, long P, float* __restrict__ part) {
    __shared__ float red[16];
    const float s = scale[0];
    float acc = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
        float r[3];
        acc += scaled_norm(*reinterpret_cast<const float4*>(m + i * 4), s, r);
    }
    const float t = sde_block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ void __launch_bounds__(256) head_apply_kernel(const float* __restrict__ m, const float* __restrict__ scale, const float* __restrict__ weight,
                                                         const float* __restrict__ part, int nblk, int B, long HW, uint8_t* __restrict__ keep,
                                                         float* __restrict__ out) {
    __shared__ double dred[256];
    const long P = (long)B * HW;
    float mean = 0.f;
    if (part) {      // fp64 mean of the norm from the partial sums, the same fixed order in every workgroup
        double a = 0.0;
        for (int i = threadIdx.x; i < nblk; i += 256) a += (double)part[i];
        dred[threadIdx.x] = a;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (threadIdx.x < off) dred[threadIdx.x] += dred[threadIdx.x + off];
            __syncthreads();
        }
        mean = (float)(dred[0] / (double)P);
    }
    const float s = scale[0], wgt = weight[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
        float r[3];
        const float n = scaled_norm(*reinterpret_cast<const float4*>(m + i * 4), s, r);
        const bool k = !part || n > mean;
        if (keep) keep[i] = k ? 1 : 0;
        const long b = i / HW, p = i - b * HW;
        float* o = out + b * 3 * HW + p;
        o[0] = k ? r[0] * wgt : 0.f;
        o[HW] = k ? r[1] * wgt : 0.f;
        o[2 * HW] = k ? r[2] * wgt : 0.f;
    }
}

__global__ void __launch_bounds__(256) head_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ m, const float* __restrict__ scale,
                                                       const float* __restrict__ weight, const uint8_t* __restrict__ keep, int B, long HW,
                                                       float* __restrict__ dm, float* __restrict__ part) {
    __shared__ float red[16];
    const long P = (long)B * HW;
    const float s = scale[0], wgt = weight[0];
    float acc = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
        const long b = i / HW, p = i - b * HW;
        const float* d = dout + b * 3 * HW + p;
        const float k = (!keep || keep[i]) ? wgt : 0.f;
        const float g0 = d[0] * k, g1 = d[HW] * k, g2 = d[2 * HW] * k;
        const float4 v = *reinterpret_cast<const float4*>(m + i * 4);
        acc += g0 * v.x + g1 * v.y + g2 * v.z;
        *reinterpret_cast<float4*>(dm + i * 4) = make_float4(g0 * s, g1 * s, g2 * s, 0.f);
    }
    const float t = sde_block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// ---------------------------------------------------------------------------------------------------------------------
// gradient of the input preparation
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) prep_bwd_kernel(const T* __restrict__ d0, const T* __restrict__ d1, int B, int C, long HW, int Cp,
                                                       float* __restrict__ dimg) {
    const long total = (long)B * C * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long p = i % HW;
        const int c = (int)((i / HW) % C);
        const long b = i / (HW * C);
        const long src = (b * HW + p) * Cp + c;
        float v = (float)d0[src];
        if (d1) v += (float)d1[src];
        dimg[i] = v;
    }
}

}  // namespace

extern "C" {

int sde_motion_resize_cat_fwd(const float* field, int h, int w, const void* skip, int B, int H, int W, int Cs, int Cr, int Cx, int dtype, void* X,
                              float* up, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(field && skip && X && up && Types::has(dtype) && B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && Cr > 0 && Cr <= Cs && Cs % V == 0 &&
                      Cx % V == 0 && Cx >= Cr + 3,
                  "sde_motion_resize_cat_fwd: bad argument (B=%d %dx%d -> %dx%d Cs=%d Cr=%d Cx=%d dtype=%d)", B, h, w, H, W, Cs, Cr, Cx, dtype);
    const int nb = sde_grid_for((long)B * H * W * (Cx / V), GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(resize_cat_fwd_kernel<T>, dim3(nb), dim3(256), 0, s, field, h, w, (const T*)skip, B, H, W, Cs, Cr, Cx, (T*)X, up);
    });
    SDE_CHECK_LAUNCH("sde_motion_resize_cat_fwd");
    return SDE_OK;
}

int sde_motion_resize_cat_bwd(const void* dX0, const void* dX1, const float* dup, int B, int H, int W, int Cx, int Cr, int Cs, int h, int w, int dtype,
                              float* dfield, void* dskip, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(dfield && Types::has(dtype) && B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && Cr > 0 && Cr <= Cs && Cs % V == 0 && Cx % V == 0 &&
                      Cx >= Cr + 3,
                  "sde_motion_resize_cat_bwd: bad argument (B=%d %dx%d -> %dx%d Cs=%d Cr=%d Cx=%d dtype=%d)", B, h, w, H, W, Cs, Cr, Cx, dtype);
    const long work = dskip ? (long)B * H * W * (Cs / V) : (long)B * h * w;
    const int nb = sde_grid_for(work, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(resize_cat_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)dX0, (const T*)dX1, dup, B, H, W, Cx, Cr, Cs, h, w, dfield, (T*)dskip);
    });
    SDE_CHECK_LAUNCH("sde_motion_resize_cat_bwd");
    return SDE_OK;
}

int sde_motion_tail_fwd(const void* o1, const void* o2, const float* w3, const float* up, long P, int ld, int mid, int dtype, float* out,
                        sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(o1 && o2 && w3 && up && out && Types::has(dtype) && P > 0 && mid > 0 && mid <= ld && ld % V == 0,
                  "sde_motion_tail_fwd: bad argument (P=%ld ld=%d mid=%d dtype=%d)", P, ld, mid, dtype);
    const int tpp = tail_tpp(2 * (ld / V));
    const int ppb = 256 / tpp;
    long nb = (P + ppb - 1) / ppb;
    if (nb > GRID_CAP) nb = GRID_CAP;
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(tail_fwd_kernel<T>, dim3((int)nb), dim3(256), 0, s, (const T*)o1, (const T*)o2, w3, up, P, ld, mid, tpp, out);
    });
    SDE_CHECK_LAUNCH("sde_motion_tail_fwd");
    return SDE_OK;
}

int sde_motion_tail_blocks(long P, int ld, int dtype) {
    const int V = sde_vec_elems(dtype);
    if (P <= 0 || ld <= 0 || ld % V) return 0;
    return tail_bwd_blocks(P, 2 * (ld / V));
}

int sde_motion_tail_bwd(const float* dout, const void* o1, const void* o2, const float* w3, long P, int ld, int mid, int dtype, void* do1, void* do2,
                        float* part, float* dw3, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(dout && o1 && o2 && w3 && do1 && do2 && part && dw3 && Types::has(dtype) && P > 0 && mid > 0 && mid <= ld && ld % V == 0,
                  "sde_motion_tail_bwd: bad argument (P=%ld ld=%d mid=%d dtype=%d)", P, ld, mid, dtype);
    const int groups2 = 2 * (ld / V);
    const int CH = tail_bwd_ch(groups2), nb = tail_bwd_blocks(P, groups2);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(tail_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, dout, (const T*)o1, (const T*)o2, w3, P, ld, mid, CH, (T*)do1, (T*)do2, part);
    });
    SDE_CHECK_LAUNCH("sde_motion_tail_bwd");
    const int n = 6 * mid;
    hipLaunchKernelGGL(tail_bwd_final_kernel, dim3((n + 3) / 4), dim3(256), 0, s, part, nb, n, dw3);
    SDE_CHECK_LAUNCH("sde_motion_tail_bwd(final)");
    return SDE_OK;
}

int sde_motion_head_blocks(long P) { return P > 0 ? head_blocks(P) : 0; }

int sde_motion_head_fwd(const float* field, const float* scale, const float* weight, int mask, int B, int H, int W, float* part, unsigned char* keep,
                        float* out, sde_stream_t stream) {
    SDE_CHECK_ARG(field && scale && weight && out && B > 0 && H > 0 && W > 0 && (!mask || (part && keep)),
                  "sde_motion_head_fwd: bad argument (B=%d H=%d W=%d mask=%d)", B, H, W, mask);
    const long P = (long)B * H * W;
    const int nb = head_blocks(P);
    hipStream_t s = (hipStream_t)stream;
    if (mask) {
        hipLaunchKernelGGL(head_sum_kernel, dim3(nb), dim3(256), 0, s, field, scale, P, part);
        SDE_CHECK_LAUNCH("sde_motion_head_fwd(sum)");
    }
    hipLaunchKernelGGL(head_apply_kernel, dim3(sde_grid_for(P, GRID_CAP)), dim3(256), 0, s, field, scale, weight, mask ? part : nullptr, nb, B, (long)H * W,
                       mask ? keep : nullptr, out);
    SDE_CHECK_LAUNCH("sde_motion_head_fwd(apply)");
    return SDE_OK;
}

int sde_motion_head_bwd(const float* dout, const float* field, const float* scale, const float* weight, const unsigned char* keep, int B, int H, int W,
                        float* dfield, float* part, sde_stream_t stream) {
    SDE_CHECK_ARG(dout && field && scale && weight && dfield && part && B > 0 && H > 0 && W > 0, "sde_motion_head_bwd: bad argument (B=%d H=%d W=%d)", B, H,
                  W);
    const long P = (long)B * H * W;
    hipLaunchKernelGGL(head_bwd_kernel, dim3(head_blocks(P)), dim3(256), 0, (hipStream_t)stream, dout, field, scale, weight, keep, B, (long)H * W, dfield, part);
    SDE_CHECK_LAUNCH("sde_motion_head_bwd");
    return SDE_OK;
}

int sde_prep_input_bwd(const void* d0, const void* d1, int B, int C, int H, int W, int Cp, int dtype, float* dimg, sde_stream_t stream) {
    SDE_CHECK_ARG(d0 && dimg && Types::has(dtype) && B > 0 && C > 0 && C <= Cp && H > 0 && W > 0, "sde_prep_input_bwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for((long)B * C * H * W, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(prep_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)d0, (const T*)d1, B, C, (long)H * W, Cp, dimg);
    });
    SDE_CHECK_LAUNCH("sde_prep_input_bwd");
    return SDE_OK;
}

}  // extern "C"
