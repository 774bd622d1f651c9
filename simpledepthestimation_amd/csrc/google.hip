// GoogleResNet's own operators on gfx950 (reference: detectron2/modeling/depth_net/GoogleResNet.py, detectron2/layers/layer_norm.py):
// everything around its convolutions that the engine in conv.hip does not already do.
//
//   randln        RandLayerNorm (layer_norm.py:L7-33): per-(sample, channel) statistics over H x W, unbiased variance, eps; in training
//                 mean and variance are each scaled by 1 + fmod(z * s, 2s) (z ~ N(0,1) per (n,c), s read from device memory so a captured
//                 graph sees later set_stddev values), s == 0 gives the factor 1 exactly.  Mean and variance are detached: backward is
//                 dx = g * gamma * r plus the dgamma / dbeta reductions.  Optional residual (added after the norm) and ReLU, pad channels zero.
//                 forward:  [stats]  per (sample, chunk) partial (sum, sum^2) of x - x[b,0,c] (a per-channel shift against cancellation)
//                           [apply]  every workgroup finalizes its sample's statistics in fp64 from the slab, then normalizes its chunk
//                 backward: [bwd]    sum of up to 3 incoming gradients, ReLU mask, dx, and partial (sum g, sum g * xhat) per (sample, chunk)
//                           [final]  dgamma / dbeta in fp64, fixed order
//   bilinear2     F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) of UpsampleBlock (L107-112); backward gathers, for
//                 every input pixel, the output taps that read it (no scatter, no atomics)
//   softplus_head F.softplus(out_conv(x)) (L103): channel 0 -> planar [B,1,H,W] fp32, flip folded in
//
// No atomics anywhere: every sum has one owner and a fixed order, so repeated runs give identical bits.
#include "vec16.h"
#include "launch.h"

namespace {

typedef SdeTypes<float, bf16_t> Types;
constexpr int GRID_CAP = SDE_GRID_CAP_16K;

constexpr int RLN_CHUNKS = SDE_RLN_CHUNKS;
constexpr int RLN_MAXC = 2048;      // LDS holds [2][RLN_MAXC] floats

__host__ __device__ __forceinline__ int rln_chunks(int HW) {
    const int n = HW / 64;
    return n < 1 ? 1 : (n > RLN_CHUNKS ? RLN_CHUNKS : n);
}

// Thread layout of the chunk kernels: TX threads walk the cch = C / V channel groups (TX = min(cch, 256)), TY = 256 / TX rows of them walk
// the pixels.  Every thread owns at most two channel groups (cch <= 512).
struct Layout {
    int cch, TX, TY, tx, ty;
    __device__ Layout(int C, int V) {
        cch = C / V;
        TX = cch < 256 ? cch : 256;
        TY = 256 / TX;
        tx = threadIdx.x % TX;
        ty = threadIdx.x / TX;
    }
};

// Write the per-thread sums (acc1/acc2 of channel groups tx, tx + 256) to LDS rows and fold the TY rows in a fixed order into
// out[c * 2 + {0, 1}] (c < C).
template <int V>
__device__ void fold_rows(const Layout& l, int C, const float (&acc1)[2][V], const float (&acc2)[2][V], float* sh, float* __restrict__ out) {
    float* sh1 = sh;
    float* sh2 = sh + RLN_MAXC;
    if (l.ty < l.TY)
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const int g = l.tx + gi * 256;
            if (g < l.cch)
#pragma unroll
                for (int e = 0; e < V; ++e) { sh1[l.ty * C + g * V + e] = acc1[gi][e]; sh2[l.ty * C + g * V + e] = acc2[gi][e]; }
        }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float s1 = 0.f, s2 = 0.f;
        for (int r = 0; r < l.TY; ++r) { s1 += sh1[r * C + c]; s2 += sh2[r * C + c]; }
        out[c * 2] = s1;
        out[c * 2 + 1] = s2;
    }
}

// forward stage 1: part[b][chunk][c] = (sum, sum^2) of x[b, p, c] - x[b, 0, c] over the chunk's pixels
template <typename T>
__global__ void __launch_bounds__(256) rln_stats_kernel(const T* __restrict__ x, int HW, int C, float* __restrict__ part) {
    constexpr int V = VecOf<T>::V;
    __shared__ float sh[2 * RLN_MAXC];
    const int b = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
    const Layout l(C, V);
    const int per = (HW + nch - 1) / nch;
    const int p0 = ch * per, p1 = min(HW, p0 + per);
    const T* xb = x + (long)b * HW * C;
    float a1[2][V], a2[2][V];
#pragma unroll
    for (int gi = 0; gi < 2; ++gi)
#pragma unroll
        for (int e = 0; e < V; ++e) { a1[gi][e] = 0.f; a2[gi][e] = 0.f; }
    if (l.ty < l.TY)
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const int g = l.tx + gi * 256;
            if (g >= l.cch) continue;
            float k[V];
            load_vec<T>(xb + g * V, k);
            for (int p = p0 + l.ty; p < p1; p += l.TY) {
                float v[V];
                load_vec<T>(xb + (long)p * C + g * V, v);
#pragma unroll
                for (int e = 0; e < V; ++e) { const float d = v[e] - k[e]; a1[gi][e] += d; a2[gi][e] += d * d; }
            }
        }
    fold_rows<V>(l, C, a1, a2, sh, part + ((long)b * RLN_CHUNKS + ch) * C * 2);
}

// forward stage 2: finalize (fp64) + apply.  Workgroup (chunk, b) recomputes sample b's statistics from the slab (nch x C partials, L2-resident)
// and normalizes its chunk; chunk 0 also stores rlnp[b][c] = (noisy mean, rstd of the noisy variance) for backward.
template <typename T>
__global__ void __launch_bounds__(256) rln_apply_kernel(const T* __restrict__ y, const T* __restrict__ res, const float* __restrict__ part,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ z,
                                                        const float* __restrict__ stddev, int train, int B, int HW, int C, int Cr, float eps, int relu,
                                                        float* __restrict__ rlnp, T* __restrict__ out) {
    constexpr int V = VecOf<T>::V;
    __shared__ float sm[RLN_MAXC], sr[RLN_MAXC];
    const int b = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
    const T* yb = y + (long)b * HW * C;
    const float s = train ? *stddev : 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        float m = 0.f, r = 0.f;
        if (c < Cr) {
            double s1 = 0.0, s2 = 0.0;
            for (int q = 0; q < nch; ++q) {
                const float* pq = part + (((long)b * RLN_CHUNKS + q) * C + c) * 2;
                s1 += pq[0];
                s2 += pq[1];
            }
            const double n = (double)HW;
            const double mean = (double)(float)yb[c] + s1 / n;
            double var = (s2 - s1 * s1 / n) / (n - 1.0);
            if (var < 0.0) var = 0.0;
            float fm = 1.f, fv = 1.f;
            if (s != 0.f) {         // layer_norm.py:L27-28; s == 0: factor 1 (the reference would compute fmod(0, 0) = NaN)
                fm = 1.f + fmodf(z[(long)b * Cr + c] * s, s * 2.f);
                fv = 1.f + fmodf(z[((long)B + b) * Cr + c] * s, s * 2.f);
            }
            m = (float)mean * fm;
            r = (float)(1.0 / sqrt((double)((float)var * fv) + (double)eps));
        }
        sm[c] = m;
        sr[c] = r;
        if (ch == 0) {
            rlnp[((long)b * C + c) * 2] = m;
            rlnp[((long)b * C + c) * 2 + 1] = r;
        }
    }
    __syncthreads();
    const int per = (HW + nch - 1) / nch;
    const int p0 = ch * per, p1 = min(HW, p0 + per);
    const int cch = C / V;
    const long n = (long)(p1 - p0) * cch;
    const long base = ((long)b * HW + p0) * C;
    for (long i = threadIdx.x; i < n; i += 256) {
        const int c0 = (int)(i % cch) * V;
        const long off = base + i * V;
        float v[V];
        load_vec<T>(y + off, v);
        float rv[V];
        if (res) load_vec<T>(res + off, rv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int c = c0 + e;
            float o = 0.f;
            if (c < Cr) {
                o = gamma[c] * ((v[e] - sm[c]) * sr[c]) + beta[c];
                if (res) o += rv[e];
                if (relu) o = fmaxf(o, 0.f);
            }
            v[e] = o;
        }
        store_vec<T>(out + off, v);
    }
}

// backward stage 1: gm = (d0 [+ d1 [+ d2]]) * relu'(out) (stored when gm_out: the residual's gradient), dx = gm * gamma * r, and
// part[b][chunk][c] = (sum gm, sum gm * xhat)
template <typename T>
__global__ void __launch_bounds__(256) rln_bwd_kernel(const T* __restrict__ d0, const T* __restrict__ d1, const T* __restrict__ d2, const T* __restrict__ out,
                                                      const T* __restrict__ y, const float* __restrict__ rlnp, const float* __restrict__ gamma, int relu,
                                                      int HW, int C, int Cr, float* __restrict__ part, T* __restrict__ gm_out, T* __restrict__ dx) {
    constexpr int V = VecOf<T>::V;
    __shared__ float sh[2 * RLN_MAXC];
    const int b = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
    const Layout l(C, V);
    const int per = (HW + nch - 1) / nch;
    const int p0 = ch * per, p1 = min(HW, p0 + per);
    const long sb = (long)b * HW * C;
    float a1[2][V], a2[2][V];
#pragma unroll
    for (int gi = 0; gi < 2; ++gi)
#pragma unroll
        for (int e = 0; e < V; ++e) { a1[gi][e] = 0.f; a2[gi][e] = 0.f; }
    if (l.ty < l.TY)
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
            const int g = l.tx + gi * 256;
            if (g >= l.cch) continue;
            float m[V], r[V], k[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int c = g * V + e;
                m[e] = rlnp[((long)b * C + c) * 2];
                r[e] = rlnp[((long)b * C + c) * 2 + 1];
                k[e] = c < Cr ? gamma[c] * r[e] : 0.f;
            }
            for (int p = p0 + l.ty; p < p1; p += l.TY) {
                const long off = sb + (long)p * C + g * V;
                float gv[V], t[V];
                load_vec<T>(d0 + off, gv);
                if (d1) {
                    load_vec<T>(d1 + off, t);
#pragma unroll
                    for (int e = 0; e < V; ++e) gv[e] += t[e];
                }
                if (d2) {
                    load_vec<T>(d2 + off, t);
#pragma unroll
                    for (int e = 0; e < V; ++e) gv[e] += t[e];
                }
                if (relu) {
                    load_vec<T>(out + off, t);
#pragma unroll
                    for (int e = 0; e < V; ++e) gv[e] = t[e] > 0.f ? gv[e] : 0.f;
                }
                if (gm_out) store_vec<T>(gm_out + off, gv);
                load_vec<T>(y + off, t);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    a1[gi][e] += gv[e];
                    a2[gi][e] += gv[e] * ((t[e] - m[e]) * r[e]);
                    t[e] = gv[e] * k[e];
                }
                store_vec<T>(dx + off, t);
            }
        }
    fold_rows<V>(l, C, a1, a2, sh, part + ((long)b * RLN_CHUNKS + ch) * C * 2);
}

// backward stage 2: dbeta[c] = sum gm, dgamma[c] = sum gm * xhat over (b, chunk) in a fixed order, fp64
__global__ void __launch_bounds__(256) rln_bwd_final_kernel(const float* __restrict__ part, int B, int nch, int C, int Cr, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int accumulate) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Cr) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < nch; ++q) {
            const float* pq = part + (((long)b * RLN_CHUNKS + q) * C + c) * 2;
            s1 += pq[0];
            s2 += pq[1];
        }
    dgamma[c] = accumulate ? dgamma[c] + (float)s2 : (float)s2;
    dbeta[c] = accumulate ? dbeta[c] + (float)s1 : (float)s1;
}

// ---------------------------------------------------------------------------------------------------------------------
// bilinear x2, align_corners=True: torch's source-index rule (upsample_bilinear2d, CPU and GPU alike):
//   src = (float)(in - 1) / (out - 1) * o, i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = clamp(src - i0, 0, 1), l0 = 1 - l1
// ---------------------------------------------------------------------------------------------------------------------
struct Tap {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Tap tap(int o, int in, float scale) {
    const float src = scale * (float)o;
    Tap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
    t.l0 = 1.f - t.l1;
    return t;
}

__device__ __forceinline__ float up_scale(int in) { return (float)(in - 1) / (float)(2 * in - 1); }

template <typename T>
__global__ void __launch_bounds__(256) bilinear2_fwd_kernel(const T* __restrict__ x, T* __restrict__ out, int B, int H, int W, int C) {
    constexpr int V = VecOf<T>::V;
    const int cch = C / V, OH = 2 * H, OW = 2 * W;
    const float sh = up_scale(H), sw = up_scale(W);
    const long total = (long)B * OH * OW * cch;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % cch);
        const long pix = i / cch;
        const int ox = (int)(pix % OW), oy = (int)((pix / OW) % OH), b = (int)(pix / ((long)OW * OH));
        const Tap ty = tap(oy, H, sh), tx = tap(ox, W, sw);
        const T* xb = x + (long)b * H * W * C + g * V;
        float v00[V], v01[V], v10[V], v11[V], o[V];
        load_vec<T>(xb + ((long)ty.i0 * W + tx.i0) * C, v00);
        load_vec<T>(xb + ((long)ty.i0 * W + tx.i1) * C, v01);
        load_vec<T>(xb + ((long)ty.i1 * W + tx.i0) * C, v10);
        load_vec<T>(xb + ((long)ty.i1 * W + tx.i1) * C, v11);
#pragma unroll
        for (int e = 0; e < V; ++e)
            o[e] = ty.l0 * (tx.l0 * v00[e] + tx.l1 * v01[e]) + ty.l1 * (tx.l0 * v10[e] + tx.l1 * v11[e]);
        store_vec<T>(out + i * V, o);
    }
}

// The output positions that read input index `i` along one axis, with their weights (at most 8: in >= 2 gives o in [2i - 3, 2i + 4];
// in == 1 gives o in {0, 1}).
__device__ __forceinline__ int gather_taps(int i, int in, float scale, int* pos, float* wt) {
    int n = 0;
    const int out = 2 * in;
    const int lo = max(0, 2 * i - 4), hi = min(out - 1, 2 * i + 5);
    for (int o = lo; o <= hi; ++o) {
        const Tap t = tap(o, in, scale);
        const float w = (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
        if ((t.i0 == i || t.i1 == i) && n < 10) { pos[n] = o; wt[n] = w; ++n; }
    }
    return n;
}

template <typename T>
__global__ void __launch_bounds__(256) bilinear2_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dx, int B, int H, int W, int C) {
    constexpr int V = VecOf<T>::V;
    const int cch = C / V, OW = 2 * W;
    const float sh = up_scale(H), sw = up_scale(W);
    const long total = (long)B * H * W * cch;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int g = (int)(i % cch);
        const long pix = i / cch;
        const int ix = (int)(pix % W), iy = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
        int py[10], px[10];
        float wy[10], wx[10];
        const int ny = gather_taps(iy, H, sh, py, wy), nx = gather_taps(ix, W, sw, px, wx);
        const T* db = dout + (long)b * 4 * H * W * C + g * V;
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
        for (int a = 0; a < ny; ++a)
            for (int c = 0; c < nx; ++c) {
                float v[V];
                load_vec<T>(db + ((long)py[a] * OW + px[c]) * C, v);
                const float w = wy[a] * wx[c];
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] += w * v[e];
            }
        store_vec<T>(dx + i * V, acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// softplus head: out[b,0,h,x] = softplus(y[b,h,x',0]) (beta 1, threshold 20), x' = x or W-1-x (flip)
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) softplus_head_fwd_kernel(const T* __restrict__ y, int B, int H, int W, int ld, int flip, float* __restrict__ out) {
    const long total = (long)B * H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % W);
        const long row = i / W;
        const int xs = flip ? W - 1 - x : x;
        const float v = (float)y[(row * W + xs) * ld];
        out[i] = v > 20.f ? v : log1pf(expf(v));
    }
}

template <typename T>
__global__ void __launch_bounds__(256) softplus_head_bwd_kernel(const T* __restrict__ y, const float* __restrict__ dout, int B, int H, int W, int ld, int flip,
                                                                T* __restrict__ dy) {
    const long total = (long)B * H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % W);
        const long row = i / W;
        const int xs = flip ? W - 1 - x : x;
        T* o = dy + (row * W + xs) * ld;
        const float v = (float)y[(row * W + xs) * ld];
        const float g = dout[i];
        if (v > 20.f) {
            o[0] = (T)g;
        } else {
            const float z = expf(v);
            o[0] = (T)(g * z / (z + 1.f));
        }
        for (int c = 1; c < ld; ++c) o[c] = (T)0.f;
    }
}

}  // namespace

extern "C" {

int sde_randln_chunks(int HW) { return rln_chunks(HW); }

int sde_randln_fwd(const void* y, const void* res, const float* gamma, const float* beta, const float* z, const float* stddev, int train, int B, int HW,
                   int C, int Cr, float eps, int relu, int dtype, float* part, float* rlnp, void* out, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(y && gamma && beta && part && rlnp && out && Types::has(dtype) && B > 0 && HW >= 2 && C > 0 && C % V == 0 && C <= RLN_MAXC &&
                      Cr > 0 && Cr <= C && (!train || (z && stddev)),
                  "sde_randln_fwd: bad argument (B=%d HW=%d C=%d Cr=%d dtype=%d train=%d)", B, HW, C, Cr, dtype, train);
    const int nch = rln_chunks(HW);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(rln_stats_kernel<T>, dim3(nch, B), dim3(256), 0, s, (const T*)y, HW, C, part);
    });
    SDE_CHECK_LAUNCH("sde_randln_fwd(stats)");
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(rln_apply_kernel<T>, dim3(nch, B), dim3(256), 0, s, (const T*)y, (const T*)res, part, gamma, beta, z, stddev, train, B, HW, C, Cr, eps, relu, rlnp,
                           (T*)out);
    });
    SDE_CHECK_LAUNCH("sde_randln_fwd(apply)");
    return SDE_OK;
}

int sde_randln_bwd(const void* d0, const void* d1, const void* d2, const void* out, const void* y, const float* rlnp, const float* gamma, int relu, int B,
                   int HW, int C, int Cr, int dtype, float* part, float* dgamma, float* dbeta, int accumulate, void* gm, void* dx, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(d0 && y && rlnp && gamma && part && dgamma && dbeta && dx && (!relu || out) && Types::has(dtype) && B > 0 && HW >= 2 && C > 0 &&
                      C % V == 0 && C <= RLN_MAXC && Cr > 0 && Cr <= C,
                  "sde_randln_bwd: bad argument (B=%d HW=%d C=%d Cr=%d dtype=%d)", B, HW, C, Cr, dtype);
    const int nch = rln_chunks(HW);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(rln_bwd_kernel<T>, dim3(nch, B), dim3(256), 0, s, (const T*)d0, (const T*)d1, (const T*)d2, (const T*)out, (const T*)y, rlnp, gamma, relu, HW, C, Cr,
                           part, (T*)gm, (T*)dx);
    });
    SDE_CHECK_LAUNCH("sde_randln_bwd");
    hipLaunchKernelGGL(rln_bwd_final_kernel, dim3((Cr + 255) / 256), dim3(256), 0, s, part, B, nch, C, Cr, dgamma, dbeta, accumulate);
    SDE_CHECK_LAUNCH("sde_randln_bwd(final)");
    return SDE_OK;
}

int sde_bilinear2_fwd(const void* x, int B, int H, int W, int C, int dtype, void* out, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(x && out && Types::has(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % V == 0, "sde_bilinear2_fwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for((long)B * 4 * H * W * (C / V), GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(bilinear2_fwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)x, (T*)out, B, H, W, C);
    });
    SDE_CHECK_LAUNCH("sde_bilinear2_fwd");
    return SDE_OK;
}

int sde_bilinear2_bwd(const void* dout, int B, int H, int W, int C, int dtype, void* dx, sde_stream_t stream) {
    const int V = sde_vec_elems(dtype);
    SDE_CHECK_ARG(dout && dx && Types::has(dtype) && B > 0 && H > 0 && W > 0 && C > 0 && C % V == 0, "sde_bilinear2_bwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for((long)B * H * W * (C / V), GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(bilinear2_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)dout, (T*)dx, B, H, W, C);
    });
    SDE_CHECK_LAUNCH("sde_bilinear2_bwd");
    return SDE_OK;
}

int sde_softplus_head_fwd(const void* y, int B, int H, int W, int ld, int flip, int dtype, float* out, sde_stream_t stream) {
    SDE_CHECK_ARG(y && out && Types::has(dtype) && B > 0 && H > 0 && W > 0 && ld >= 1, "sde_softplus_head_fwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for((long)B * H * W, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(softplus_head_fwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)y, B, H, W, ld, flip, out);
    });
    SDE_CHECK_LAUNCH("sde_softplus_head_fwd");
    return SDE_OK;
}

int sde_softplus_head_bwd(const void* y, const float* dout, int B, int H, int W, int ld, int flip, int dtype, void* dy, sde_stream_t stream) {
    SDE_CHECK_ARG(y && dout && dy && Types::has(dtype) && B > 0 && H > 0 && W > 0 && ld >= 1, "sde_softplus_head_bwd: bad argument (dtype %d)", dtype);
    const int nb = sde_grid_for((long)B * H * W, GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(softplus_head_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)y, dout, B, H, W, ld, flip, (T*)dy);
    });
    SDE_CHECK_LAUNCH("sde_softplus_head_bwd");
    return SDE_OK;
}

}  // extern "C"
