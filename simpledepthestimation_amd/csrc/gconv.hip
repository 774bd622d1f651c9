// Grouped 3x3 convolution (Cin == Cout == C, G groups, padding 1, stride 1 or 2, no bias, no activation): the 3x3 of a ResNeXt bottleneck
// (torchvision's Bottleneck with groups > 1; reference encoder list: detectron2/modeling/depth_net/BTSNet.py:L278-313).
//
// With Cg = C / G channels per group the layer is C / S independent dense S -> S convolutions, S = max(Cg, 16) (a "super-group"): for Cg < 16
// the S x 9 x S weight tile is block diagonal with exact zeros off the blocks, so an MFMA tile executes 2 M C 9 S FLOPs for 2 M C 9 Cg useful
// ones (at most 4 x) instead of the 2 M C 9 C of a dense layer with a block-diagonal weight.
//
// Forward and data gradient are one kernel.  A workgroup (4 waves) owns RB = 16 or 32 output channels of one super-group and 4 * bpw blocks of 16
// output pixels (bpw <= 16, chosen from the shape so that a layer has about 1024 workgroups).  It stages its [RB][9][S] weight tile into LDS
// straight from the fp32 master weight (either memory order: [C][Cg][3][3] or the trainer's [C][3][3][Cg]), converting on the way -- no packed
// copy, no pack launch; the data gradient stages the transposed blocks.  Per pixel block a wave walks K = (taps) x S in steps of four 16-byte
// chunks:
//
//   D[channel][pixel] += A[channel][k] B[k][pixel]      bf16: v_mfma_f32_16x16x32_bf16, fp32: 4 x v_mfma_f32_16x16x4_f32
//
// A from LDS (one 16-byte read per lane), B one 16-byte global load per lane of the tap-shifted pixel (the nine taps of a pixel hit the same
// cache lines; the floor of the layer is one HBM read of x and one write of y), zeros outside the image and in the K padding; all loads of a
// pixel block are issued before its first MFMA.
// Data gradient of a stride-2 layer: the pixels of dx are enumerated by parity class (row parity, column parity); a class has 1, 2, 2 or 4 live
// taps, uniform over a pixel block, so only those are walked -- no zero-inserted image, no dead taps.
// Statistics (forward): per workgroup (sum, sum of squares) of the STORED outputs, [tiles + SDE_REDUCE_ROWS][C][2], the slab sde_bn_finalize reads.
//
// Weight gradient: per super-group and tap dW = dz^T x_shifted, reduced over pixels.  A workgroup takes a range of 32-pixel (fp32: 16) K steps: the
// dz tile and the nine shifted x tiles go through LDS transposed (pixel-contiguous rows), its 9 (S/16)^2 MFMA tiles are spread over the four waves,
// and it writes an fp32 partial slab [range][C][9][S].  A second launch sums the ranges in a fixed order and writes the diagonal Cg x Cg blocks
// into the gradient (OIHW or OHWI order, overwrite or accumulate): no floating-point atomics, bit-reproducible.
#include "common.h"
#include "sde_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float gc_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 gc_bf16x8;

constexpr int GC_THREADS = 256, GC_MAX_BPW = 16, GC_TARGET_WGS = 1024;
constexpr long GC_SLAB_BUDGET = 16L << 20;            // bytes of weight-gradient partials per layer

template <typename T> struct GcT;
template <> struct GcT<bf16_t> {
    static __device__ __forceinline__ gc_f32x4 mma(uint4 a, uint4 b, gc_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gc_bf16x8, a), __builtin_bit_cast(gc_bf16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ void store4(unsigned char* dst, float* v) {        // stores and leaves the stored (rounded) values in v
        typedef __attribute__((ext_vector_type(2))) __bf16 v2;
        const v2 lo{(__bf16)v[0], (__bf16)v[1]}, hi{(__bf16)v[2], (__bf16)v[3]};
        *reinterpret_cast<uint2*>(dst) = uint2{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
        v[0] = (float)lo[0]; v[1] = (float)lo[1]; v[2] = (float)hi[0]; v[3] = (float)hi[1];
    }
    static __device__ __forceinline__ bf16_t from(float v) { return (bf16_t)v; }
};
template <> struct GcT<float> {
    static __device__ __forceinline__ gc_f32x4 mma(uint4 a, uint4 b, gc_f32x4 c) {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.x), __builtin_bit_cast(float, b.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.y), __builtin_bit_cast(float, b.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.z), __builtin_bit_cast(float, b.z), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.w), __builtin_bit_cast(float, b.w), c, 0, 0, 0);
        return c;
    }
    static __device__ __forceinline__ void store4(unsigned char* dst, float* v) { *reinterpret_cast<float4*>(dst) = float4{v[0], v[1], v[2], v[3]}; }
    static __device__ __forceinline__ float from(float v) { return v; }
};

// ---------------------------------------------------------------------------------------------------------------
// forward / data gradient
// ---------------------------------------------------------------------------------------------------------------
struct GconvP {
    const void* src;      // [B][SH][SW][C]: x (forward) or dz (data gradient)
    const float* w;       // fp32 master weight, [C][Cg][3][3] or (ohwi) [C][3][3][Cg]
    void* dst;            // [B][DH][DW][C]: y or dx
    float* stats;         // forward only, may be null
    int B, SH, SW, DH, DW, C, Cg, stride, ohwi, bpw;
    int cls_end[4];       // pixel blocks: running ends of the four parity classes (one class unless this is a stride-2 data gradient)
    int cls_h[4], cls_w[4];
};

// MODE 0: forward, 1: data gradient of a stride-1 layer, 2: data gradient of a stride-2 layer (parity classes)
template <typename T, int S, int CB, int MODE>
__global__ void __launch_bounds__(GC_THREADS) gconv3x3_kernel(const GconvP p) {
    constexpr bool DGRAD = MODE != 0, split = MODE == 2;
    constexpr int ES = sizeof(T), CHK = 16 / ES, CPT = S / CHK;       // channels per 16-byte chunk, chunks per tap
    constexpr int NST = split ? CPT : (9 * CPT + 3) / 4;              // K steps of a pixel block: nine taps, or the four of the largest parity class
    constexpr int RB = 16 * CB, RS = 9 * S + CHK;                     // rows of the weight tile, its row stride in elements (+16 bytes: bank spread)
    __shared__ __attribute__((aligned(16))) T sW[RB * RS];
    __shared__ float red[4][RB][2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int sg = blockIdx.y, row0 = blockIdx.z * RB, ch0 = sg * S;
    const int Cg = p.Cg;

    // ---- weight tile [row][tap][col], pairs of columns per thread: row = channel this launch produces, col = channel it reduces over
    for (int id = tid; id < RB * 9 * (S / 2); id += GC_THREADS) {
        const int i = (id % (S / 2)) * 2, tap = (id / (S / 2)) % 9, o = id / (S / 2 * 9), ol = row0 + o;
        float v0 = 0.f, v1 = 0.f;
        if (ol / Cg == i / Cg) {                                     // same group (Cg is even: so is the pair's second column)
            // forward: W[co = row][ci = col]; data gradient: W[co = col][ci = row]
            const int co = ch0 + (DGRAD ? i : ol), icg = (DGRAD ? ol : i) % Cg;
            const size_t a0 = p.ohwi ? ((size_t)co * 9 + tap) * Cg + icg : ((size_t)co * Cg + icg) * 9 + tap;
            const size_t step = DGRAD ? (size_t)9 * Cg : (p.ohwi ? (size_t)1 : (size_t)9);       // to the pair's second column: co + 1 or icg + 1
            v0 = p.w[a0]; v1 = p.w[a0 + step];
        }
        T* d = &sW[o * RS + tap * S + i];
        d[0] = GcT<T>::from(v0); d[1] = GcT<T>::from(v1);
    }
    __syncthreads();

    const unsigned char* sb = static_cast<const unsigned char*>(p.src);
    float s1[CB][4], s2[CB][4];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) s1[cb][e] = s2[cb][e] = 0.f;

    const int total = p.cls_end[3];
    for (int it = 0; it < p.bpw; ++it) {
        const int gb = (blockIdx.x * p.bpw + it) * 4 + wave;        // wave-uniform
        if (gb >= total) break;
        // ---- parity class of this pixel block and its live taps
        int cls = 0;
        if (split) cls = gb < p.cls_end[0] ? 0 : gb < p.cls_end[1] ? 1 : gb < p.cls_end[2] ? 2 : 3;
        const int cstart = cls == 0 ? 0 : p.cls_end[cls - 1];
        const int Hc = p.cls_h[cls], Wc = p.cls_w[cls];
        const int pa = split ? (cls >> 1) : 0, pb = split ? (cls & 1) : 0, cs = split ? 2 : 1;
        const int nky = split ? (pa ? 2 : 1) : 3, ky0 = split ? (pa ? 0 : 1) : 0, kys = split ? 2 : 1;
        const int nkx = split ? (pb ? 2 : 1) : 3, kx0 = split ? (pb ? 0 : 1) : 0, kxs = split ? 2 : 1;
        const int nchunks = nky * nkx * CPT, nsteps = (nchunks + 3) >> 2;
        // ---- this lane's pixel
        const unsigned idx = (unsigned)(gb - cstart) * 16u + li, per = (unsigned)(Hc * Wc);        // (host: fewer than 2^31 pixels)
        const bool pvalid = idx < (unsigned)p.B * per;
        const int n = (int)(idx / per), rem = (int)(idx - (unsigned)n * per), i = rem / Wc, j = rem - i * Wc;
        const int r = i * cs + pa, c = j * cs + pb;

        auto chunk = [&](int s, int& koff) -> uint4 {                // B operand of step s (zeros: K padding, outside the image) and A's K offset
            const int q = 4 * s + lg, t = q / CPT, cc = q - t * CPT;
            const int ty = t / nkx, tx = t - ty * nkx, ky = ky0 + kys * ty, kx = kx0 + kxs * tx;
            koff = q < nchunks ? (ky * 3 + kx) * S + cc * CHK : -1;
            int sr, sc;
            if (DGRAD) { sr = r + 1 - ky; sc = c + 1 - kx; if (split) { sr >>= 1; sc >>= 1; } }
            else { sr = r * p.stride - 1 + ky; sc = c * p.stride - 1 + kx; }
            const bool ok = pvalid && q < nchunks && sr >= 0 && sr < p.SH && sc >= 0 && sc < p.SW;
            return ok ? *reinterpret_cast<const uint4*>(sb + ((((size_t)n * p.SH + sr) * p.SW + sc) * p.C + ch0 + cc * CHK) * ES) : uint4{0u, 0u, 0u, 0u};
        };

        gc_f32x4 acc[CB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[cb] = gc_f32x4{0.f, 0.f, 0.f, 0.f};
        // every load of the block is in flight before its first MFMA: one load per wave at a time left the kernel waiting on memory latency
        uint4 b[NST];
        int koff[NST];
#pragma unroll
        for (int s = 0; s < NST; ++s) {
            if (!split || s < nsteps) b[s] = chunk(s, koff[s]);
            else { b[s] = uint4{0u, 0u, 0u, 0u}; koff[s] = -1; }
        }
#pragma unroll
        for (int s = 0; s < NST; ++s) {
            if (!split || s < nsteps) {                              // wave-uniform
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    const uint4 a = koff[s] >= 0 ? *reinterpret_cast<const uint4*>(&sW[(cb * 16 + li) * RS + koff[s]]) : uint4{0u, 0u, 0u, 0u};
                    acc[cb] = GcT<T>::mma(a, b[s], acc[cb]);
                }
            }
        }
        // ---- epilogue: lane = (pixel li, channels 4 lg .. 4 lg + 3 of every 16-row block)
        if (pvalid) {
            unsigned char* db = static_cast<unsigned char*>(p.dst) + ((((size_t)n * p.DH + r) * p.DW + c) * p.C + ch0 + row0 + 4 * lg) * ES;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                float v[4] = {acc[cb][0], acc[cb][1], acc[cb][2], acc[cb][3]};
                GcT<T>::store4(db + cb * 16 * ES, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) { s1[cb][e] += v[e]; s2[cb][e] += v[e] * v[e]; }
            }
        }
    }

    if (DGRAD || !p.stats) return;
    // ---- statistics: the 16 pixel lanes of a row, then the four waves, in a fixed order
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = s1[cb][e], b2 = s2[cb][e];
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) { a += __shfl_xor(a, m); b2 += __shfl_xor(b2, m); }
            if (li == 0) { red[wave][cb * 16 + 4 * lg + e][0] = a; red[wave][cb * 16 + 4 * lg + e][1] = b2; }
        }
    __syncthreads();
    if (tid < RB) {
        const float a = ((red[0][tid][0] + red[1][tid][0]) + red[2][tid][0]) + red[3][tid][0];
        const float b2 = ((red[0][tid][1] + red[1][tid][1]) + red[2][tid][1]) + red[3][tid][1];
        float* o = p.stats + ((size_t)blockIdx.x * p.C + ch0 + row0 + tid) * 2;
        o[0] = a; o[1] = b2;
    }
}

struct GcGeom { int S, CB, nsg, zb; };
// rows of the weight tile per workgroup: the whole super-group up to 32 rows in bf16, 16 rows in fp32 (LDS: at most 32 x 584 x 2 = 16 x 580 x 4 = 37 KB)
static GcGeom gc_geom(int C, int G, int dtype) {
    GcGeom g;
    const int Cg = C / G;
    g.S = Cg < 16 ? 16 : Cg;
    g.CB = (dtype == SDE_BF16 && g.S >= 32) ? 2 : 1;
    g.nsg = C / g.S;
    g.zb = g.S / (16 * g.CB);
    return g;
}
static int gc_bpw(long nblk, const GcGeom& g) {
    const long b = nblk * g.nsg * g.zb / (4L * GC_TARGET_WGS);
    return b < 1 ? 1 : b > GC_MAX_BPW ? GC_MAX_BPW : (int)b;
}
static bool gc_shape_ok(int C, int G) {
    if (C <= 0 || G <= 0 || C % G || C % 16) return false;
    const int Cg = C / G;
    return Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32 || Cg == 64;
}

template <typename T, int MODE>
static void gconv_launch(const GconvP& p, const GcGeom& g, int tiles, hipStream_t s) {
    const dim3 grid(tiles, g.nsg, g.zb), block(GC_THREADS);
    if constexpr (sizeof(T) == 2) {                       // (gc_geom: two 16-row blocks per workgroup in bf16 from S = 32 on, one in fp32)
        if (g.S == 16) hipLaunchKernelGGL((gconv3x3_kernel<T, 16, 1, MODE>), grid, block, 0, s, p);
        else if (g.S == 32) hipLaunchKernelGGL((gconv3x3_kernel<T, 32, 2, MODE>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((gconv3x3_kernel<T, 64, 2, MODE>), grid, block, 0, s, p);
    } else {
        if (g.S == 16) hipLaunchKernelGGL((gconv3x3_kernel<T, 16, 1, MODE>), grid, block, 0, s, p);
        else if (g.S == 32) hipLaunchKernelGGL((gconv3x3_kernel<T, 32, 1, MODE>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((gconv3x3_kernel<T, 64, 1, MODE>), grid, block, 0, s, p);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------------------------
struct GwgradP {
    const void* x;        // [B][IH][IW][C]
    const void* dz;       // [B][OH][OW][C]
    float* slab;          // [ranges][C][9][S]
    int B, IH, IW, OH, OW, C, stride, nk, kper;
};

template <typename T, int S>
__global__ void __launch_bounds__(GC_THREADS) gconv3x3_wgrad_kernel(const GwgradP p) {
    constexpr int ES = sizeof(T), CHK = 16 / ES, CPT = S / CHK, KP = 4 * CHK;       // pixels per K step
    constexpr int RSP = KP + CHK;                                                   // row stride in elements (80 bytes)
    constexpr int CBS = S / 16, NBLK = 9 * CBS * CBS, NACC = (NBLK + 3) / 4;
    constexpr int JOBS = 10 * KP * CPT, NJ = (JOBS + GC_THREADS - 1) / GC_THREADS;
    __shared__ __attribute__((aligned(16))) T sT[10 * S * RSP];                     // [dz, x tap 0 .. 8][channel][pixel]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int ch0 = blockIdx.y * S;
    const long M = (long)p.B * p.OH * p.OW;
    const unsigned char* xb = static_cast<const unsigned char*>(p.x);
    const unsigned char* zb = static_cast<const unsigned char*>(p.dz);

    gc_f32x4 acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = gc_f32x4{0.f, 0.f, 0.f, 0.f};

    uint4 rg[NJ];
    auto load_step = [&](int ks) {
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int id = tid + k * GC_THREADS, cc = id % CPT, pix = (id / CPT) % KP, which = id / (CPT * KP);
            const long m = (long)ks * KP + pix;
            uint4 v = uint4{0u, 0u, 0u, 0u};
            if (id < JOBS && m < M) {
                const int ow = (int)(m % p.OW), oh = (int)((m / p.OW) % p.OH), n = (int)(m / ((long)p.OW * p.OH));
                if (which == 0) {
                    v = *reinterpret_cast<const uint4*>(zb + ((size_t)m * p.C + ch0 + cc * CHK) * ES);
                } else {
                    const int tap = which - 1, ih = oh * p.stride - 1 + tap / 3, iw = ow * p.stride - 1 + tap % 3;
                    if (ih >= 0 && ih < p.IH && iw >= 0 && iw < p.IW)
                        v = *reinterpret_cast<const uint4*>(xb + ((((size_t)n * p.IH + ih) * p.IW + iw) * p.C + ch0 + cc * CHK) * ES);
                }
            }
            rg[k] = v;
        }
    };

    const int k0 = blockIdx.x * p.kper, k1 = min(p.nk, k0 + p.kper);
    if (k0 < k1) load_step(k0);
    for (int ks = k0; ks < k1; ++ks) {
        __syncthreads();                                  // every wave is done with the previous step's tiles
#pragma unroll
        for (int k = 0; k < NJ; ++k) {
            const int id = tid + k * GC_THREADS, cc = id % CPT, pix = (id / CPT) % KP, which = id / (CPT * KP);
            if (id < JOBS) {
                const T* e = reinterpret_cast<const T*>(&rg[k]);
#pragma unroll
                for (int q = 0; q < CHK; ++q) sT[(which * S + cc * CHK + q) * RSP + pix] = e[q];       // transposed: pixel-contiguous rows
            }
        }
        __syncthreads();
        if (ks + 1 < k1) load_step(ks + 1);
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            const int jb = wave + 4 * a;                  // wave-uniform
            if (jb < NBLK) {
                const int tap = jb / (CBS * CBS), rem = jb - tap * (CBS * CBS), cbr = rem / CBS, cbc = rem - cbr * CBS;
                const uint4 av = *reinterpret_cast<const uint4*>(&sT[(cbr * 16 + li) * RSP + lg * CHK]);
                const uint4 bv = *reinterpret_cast<const uint4*>(&sT[((tap + 1) * S + cbc * 16 + li) * RSP + lg * CHK]);
                acc[a] = GcT<T>::mma(av, bv, acc[a]);
            }
        }
    }
    // ---- partial slab: D[row = dz channel 4 lg + e][col = x channel li] of every tile
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        const int jb = wave + 4 * a;
        if (jb < NBLK) {
            const int tap = jb / (CBS * CBS), rem = jb - tap * (CBS * CBS), cbr = rem / CBS, cbc = rem - cbr * CBS;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                p.slab[(((size_t)blockIdx.x * p.C + ch0 + cbr * 16 + 4 * lg + e) * 9 + tap) * S + cbc * 16 + li] = acc[a][e];
        }
    }
}

__global__ void __launch_bounds__(256) gconv3x3_wreduce_kernel(const float* __restrict__ slab, int ranges, int C, int Cg, int S, int flags, float* __restrict__ dw) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)C * Cg * 9) return;
    const int tap = (int)(e % 9), icg = (int)((e / 9) % Cg), co = (int)(e / (9L * Cg));
    const int col = ((co % S) / Cg) * Cg + icg;           // the diagonal block of this output channel inside its super-group tile
    float sum = 0.f;
    for (int r = 0; r < ranges; ++r) sum += slab[(((size_t)r * C + co) * 9 + tap) * S + col];
    const size_t d = (flags & SDE_WREDUCE_OHWI) ? ((size_t)co * 9 + tap) * Cg + icg : (size_t)e;
    dw[d] = (flags & SDE_WREDUCE_ACCUMULATE) ? dw[d] + sum : sum;
}

struct GwPlan { int S, nsg, kp, nk, kper, ranges; };
static GwPlan gw_plan(int B, int OH, int OW, int C, int G, int dtype) {
    GwPlan w;
    const int Cg = C / G;
    w.S = Cg < 16 ? 16 : Cg;
    w.nsg = C / w.S;
    w.kp = dtype == SDE_BF16 ? 32 : 16;
    w.nk = sde_cdiv((long)B * OH * OW, w.kp);
    long want = GC_TARGET_WGS / w.nsg;
    const long cap = GC_SLAB_BUDGET / (36L * C * w.S);     // ranges the slab budget allows
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    if (want > w.nk) want = w.nk;
    w.kper = sde_cdiv(w.nk, want);
    w.ranges = sde_cdiv(w.nk, w.kper);
    return w;
}

static int gc_check(const char* name, int B, int H, int W, int C, int G, int stride, int dtype) {
    SDE_CHECK_ARG(dtype == SDE_F32 || dtype == SDE_BF16, "%s: fp32 or bf16 storage only (dtype %d)", name, dtype);
    SDE_CHECK_ARG(gc_shape_ok(C, G), "%s: C=%d G=%d is not supported (C %% 16 == 0 and C / G in {4, 8, 16, 32, 64})", name, C, G);
    SDE_CHECK_ARG(stride == 1 || stride == 2, "%s: stride %d is not supported (1 or 2)", name, stride);
    SDE_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: bad shape [%d,%d,%d,%d]", name, B, H, W, C);
    SDE_CHECK_ARG((long)B * H * W * C < 0x7fffffffL, "%s: tensors must have fewer than 2^31 elements", name);
    return SDE_OK;
}

}  // namespace

static inline int gc_out(int n, int stride) { return (n - 1) / stride + 1; }      // (n + 2 - 3) / stride + 1

extern "C" int sde_gconv3x3_stats_rows(int B, int H, int W, int C, int G, int stride, int dtype) {
    if (gc_check("sde_gconv3x3_stats_rows", B, H, W, C, G, stride, dtype) != SDE_OK) return -1;
    const GcGeom g = gc_geom(C, G, dtype);
    const long nblk = sde_cdiv((long)B * gc_out(H, stride) * gc_out(W, stride), 16);
    return sde_cdiv(nblk, 4L * gc_bpw(nblk, g));
}

extern "C" int sde_gconv3x3_fwd(const void* x, const float* w, int w_ohwi, int B, int H, int W, int C, int G, int stride, int dtype, void* y, float* stats,
                                sde_stream_t stream) {
    SDE_CHECK_ARG(x && w && y, "sde_gconv3x3_fwd: null pointer");
    if (int rc = gc_check("sde_gconv3x3_fwd", B, H, W, C, G, stride, dtype)) return rc;
    const GcGeom g = gc_geom(C, G, dtype);
    GconvP p;
    p.src = x; p.w = w; p.dst = y; p.stats = stats;
    p.B = B; p.SH = H; p.SW = W; p.DH = gc_out(H, stride); p.DW = gc_out(W, stride); p.C = C; p.Cg = C / G; p.stride = stride; p.ohwi = w_ohwi ? 1 : 0;
    const long nblk = sde_cdiv((long)B * p.DH * p.DW, 16);
    p.bpw = gc_bpw(nblk, g);
    for (int k = 0; k < 4; ++k) { p.cls_end[k] = (int)nblk; p.cls_h[k] = p.DH; p.cls_w[k] = p.DW; }
    const int tiles = sde_cdiv(nblk, 4L * p.bpw);
    if (dtype == SDE_BF16) gconv_launch<bf16_t, 0>(p, g, tiles, (hipStream_t)stream); else gconv_launch<float, 0>(p, g, tiles, (hipStream_t)stream);
    SDE_CHECK_LAUNCH("sde_gconv3x3_fwd");
    return SDE_OK;
}

extern "C" int sde_gconv3x3_dgrad(const void* dz, const float* w, int w_ohwi, int B, int H, int W, int C, int G, int stride, int dtype, void* dx,
                                  sde_stream_t stream) {
    SDE_CHECK_ARG(dz && w && dx, "sde_gconv3x3_dgrad: null pointer");
    if (int rc = gc_check("sde_gconv3x3_dgrad", B, H, W, C, G, stride, dtype)) return rc;
    const GcGeom g = gc_geom(C, G, dtype);
    GconvP p;
    p.src = dz; p.w = w; p.dst = dx; p.stats = nullptr;
    p.B = B; p.SH = gc_out(H, stride); p.SW = gc_out(W, stride); p.DH = H; p.DW = W; p.C = C; p.Cg = C / G; p.stride = stride; p.ohwi = w_ohwi ? 1 : 0;
    long end = 0;
    for (int k = 0; k < 4; ++k) {
        // stride 2: class k = (row parity, column parity) holds the pixels (2 i + a, 2 j + b) of dx; stride 1: one class, every pixel
        const int a = k >> 1, b = k & 1;
        p.cls_h[k] = stride == 2 ? (H + 1 - a) / 2 : H;
        p.cls_w[k] = stride == 2 ? (W + 1 - b) / 2 : W;
        if (stride == 2 || k == 0) end += sde_cdiv((long)B * p.cls_h[k] * p.cls_w[k], 16);
        p.cls_end[k] = (int)end;
    }
    p.bpw = gc_bpw(end, g);
    const int tiles = sde_cdiv(end, 4L * p.bpw);
    hipStream_t s = (hipStream_t)stream;
    if (stride == 2) { if (dtype == SDE_BF16) gconv_launch<bf16_t, 2>(p, g, tiles, s); else gconv_launch<float, 2>(p, g, tiles, s); }
    else { if (dtype == SDE_BF16) gconv_launch<bf16_t, 1>(p, g, tiles, s); else gconv_launch<float, 1>(p, g, tiles, s); }
    SDE_CHECK_LAUNCH("sde_gconv3x3_dgrad");
    return SDE_OK;
}

extern "C" size_t sde_gconv3x3_wgrad_ws_bytes(int B, int H, int W, int C, int G, int stride, int dtype) {
    if (gc_check("sde_gconv3x3_wgrad_ws_bytes", B, H, W, C, G, stride, dtype) != SDE_OK) return 0;
    const GwPlan w = gw_plan(B, gc_out(H, stride), gc_out(W, stride), C, G, dtype);
    return (size_t)w.ranges * C * 9 * w.S * sizeof(float);
}

extern "C" int sde_gconv3x3_wgrad(const void* x, const void* dz, int B, int H, int W, int C, int G, int stride, int dtype, float* ws, size_t ws_bytes,
                                  float* dw, int flags, sde_stream_t stream) {
    SDE_CHECK_ARG(x && dz && ws && dw, "sde_gconv3x3_wgrad: null pointer");
    if (int rc = gc_check("sde_gconv3x3_wgrad", B, H, W, C, G, stride, dtype)) return rc;
    SDE_CHECK_ARG((flags & ~(SDE_WREDUCE_ACCUMULATE | SDE_WREDUCE_OHWI)) == 0, "sde_gconv3x3_wgrad: bad flags %d", flags);
    GwgradP p;
    p.x = x; p.dz = dz; p.slab = ws;
    p.B = B; p.IH = H; p.IW = W; p.OH = gc_out(H, stride); p.OW = gc_out(W, stride); p.C = C; p.stride = stride;
    const GwPlan w = gw_plan(B, p.OH, p.OW, C, G, dtype);
    SDE_CHECK_ARG(ws_bytes >= (size_t)w.ranges * C * 9 * w.S * sizeof(float), "sde_gconv3x3_wgrad: workspace of %zu bytes is too small (sde_gconv3x3_wgrad_ws_bytes)", ws_bytes);
    p.nk = w.nk; p.kper = w.kper;
    const dim3 grid(w.ranges, w.nsg), block(GC_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SDE_BF16) {
        if (w.S == 16) hipLaunchKernelGGL((gconv3x3_wgrad_kernel<bf16_t, 16>), grid, block, 0, s, p);
        else if (w.S == 32) hipLaunchKernelGGL((gconv3x3_wgrad_kernel<bf16_t, 32>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((gconv3x3_wgrad_kernel<bf16_t, 64>), grid, block, 0, s, p);
    } else {
        if (w.S == 16) hipLaunchKernelGGL((gconv3x3_wgrad_kernel<float, 16>), grid, block, 0, s, p);
        else if (w.S == 32) hipLaunchKernelGGL((gconv3x3_wgrad_kernel<float, 32>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((gconv3x3_wgrad_kernel<float, 64>), grid, block, 0, s, p);
    }
    SDE_CHECK_LAUNCH("sde_gconv3x3_wgrad");
    const long n = (long)C * (C / G) * 9;
    hipLaunchKernelGGL(gconv3x3_wreduce_kernel, dim3(sde_cdiv(n, 256)), dim3(256), 0, s, ws, w.ranges, C, C / G, w.S, flags, dw);
    SDE_CHECK_LAUNCH("sde_gconv3x3_wgrad (reduce)");
    return SDE_OK;
}
