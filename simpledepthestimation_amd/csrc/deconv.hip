// ConvTranspose2d(Cin, Cout, 3, stride 2, padding 1, output_padding 1) forward: GoogleResNetv2's five up-sampling layers (reference:
// detectron2/modeling/depth_net/GoogleResNetv2.py:L42-44 deconv3x3, L127-138 UpsampleBlock).
//
// As the data gradient of its adjoint stride-2 convolution (SDE_SRC_ZEROINS) the layer multiplies nine taps per OUTPUT pixel against an image that is
// three quarters zeros.  Split by output parity it is four small convolutions of the stored input, nine tap products per INPUT pixel:
//
//   y[2i,   2j  ] = W11 x[i,j]
//   y[2i,   2j+1] = W12 x[i,j] + W10 x[i,j+1]
//   y[2i+1, 2j  ] = W21 x[i,j] + W01 x[i+1,j]
//   y[2i+1, 2j+1] = W22 x[i,j] + W20 x[i,j+1] + W02 x[i+1,j] + W00 x[i+1,j+1]            (x[H,.] = x[.,W] = 0)
//
// Operand: [ldy][3][3][C], taps flipped -- sde_pack_weight(for_dgrad = 1) of the adjoint convolution, whose OIHW weight IS the ConvTranspose2d weight
// [Cin,Cout,3,3].  In its tap coordinates (ty,tx) a tap feeds output parity (ty != 1, tx != 1) and reads the input at (+[ty == 2], +[tx == 2]).
//
// A 256-thread workgroup takes an 8 x 16 tile of input pixels and 16 CB output channels.  Per K step (64 bytes of channels: 32 bf16 / 16 fp32) it
// stages the (8+1) x (16+1) halo tile and the nine taps' weight slices in LDS, pixel- and channel-row-major with 64-byte rows, so every MFMA operand is
// one 16-byte read per lane of a contiguous 1 KB (2-way bank conflicts under ds_read_b128's lane groups; an XOR swizzle of the four slots is a follow-up).  The global loads of K step s + 1 are issued into registers before the MFMAs of
// step s, so the loop does not wait a memory latency per step (the 512-channel layer runs 16 steps).  A wave owns two tile rows: 6 B reads + 9 CB A reads feed 18 CB MFMAs
//
//   bf16: v_mfma_f32_16x16x32_bf16, fp32: 4 x v_mfma_f32_16x16x4_f32 (the engine's fp32 arithmetic):  D[co][pixel] += A[co][k] B[k][pixel]
//
// into 2 rows x 4 parities x CB accumulators.  Epilogue: a lane holds 4 consecutive output channels of one input pixel's 2 x 2 output block: bias,
// activation, and 8- / 16-byte stores straight into the interleaved NHWC rows; channels >= Cout are stored as zeros.
#include "common.h"
#include "sde_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float dc_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 dc_bf16x8;

constexpr int DC_TH = 8, DC_TW = 16, DC_HH = DC_TH + 1, DC_HW = DC_TW + 1, DC_THREADS = 256;
constexpr int DC_XCHUNKS = DC_HH * DC_HW * 4;      // 16-byte chunks of one K step's halo tile

struct DeconvP {
    const void* x;        // [B][H][W][C]
    const void* w;        // [ldy][3][3][C]
    const float* bias;    // [Cout] or null
    void* y;              // [B][2H][2W][ldy]
    int B, H, W, C, Cout, ldy, act;
    int tiles_h, tiles_w;
};

template <typename T> struct DcT;
template <> struct DcT<bf16_t> {
    static __device__ __forceinline__ dc_f32x4 mma(uint4 a, uint4 b, dc_f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dc_bf16x8, a), __builtin_bit_cast(dc_bf16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ void store4(unsigned char* dst, const float* v) {
        typedef __attribute__((ext_vector_type(2))) __bf16 v2;
        *reinterpret_cast<uint2*>(dst) = uint2{__builtin_bit_cast(unsigned, v2{(__bf16)v[0], (__bf16)v[1]}), __builtin_bit_cast(unsigned, v2{(__bf16)v[2], (__bf16)v[3]})};
    }
};
template <> struct DcT<float> {
    static __device__ __forceinline__ dc_f32x4 mma(uint4 a, uint4 b, dc_f32x4 c) {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.x), __builtin_bit_cast(float, b.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.y), __builtin_bit_cast(float, b.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.z), __builtin_bit_cast(float, b.z), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a.w), __builtin_bit_cast(float, b.w), c, 0, 0, 0);
        return c;
    }
    static __device__ __forceinline__ void store4(unsigned char* dst, const float* v) { *reinterpret_cast<float4*>(dst) = float4{v[0], v[1], v[2], v[3]}; }
};

template <typename T, int CB>
__global__ void __launch_bounds__(DC_THREADS) deconv3x3s2_kernel(const DeconvP p) {
    constexpr int ES = sizeof(T), CHK = 16 / ES, KSTEP = 4 * CHK;       // channels per 16-byte chunk and per K step
    constexpr int NCO = CB * 16, WCHUNKS = 9 * NCO * 4;
    __shared__ __attribute__((aligned(16))) unsigned char sX[DC_XCHUNKS * 16];     // [9 x 17 pixels][KSTEP]
    __shared__ __attribute__((aligned(16))) unsigned char sW[WCHUNKS * 16];        // [9 taps][NCO][KSTEP]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int per_img = p.tiles_h * p.tiles_w;
    const int t = blockIdx.x, n = t / per_img, rem = t - n * per_img;
    const int th = rem / p.tiles_w, tw = rem - th * p.tiles_w;
    const int i0 = th * DC_TH, j0 = tw * DC_TW, co0 = blockIdx.y * NCO;
    const unsigned char* xg = static_cast<const unsigned char*>(p.x);
    const unsigned char* wg = static_cast<const unsigned char*>(p.w);

    dc_f32x4 acc[2][4][CB];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) acc[rr][q][cb] = dc_f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- per-thread staging plan: the chunks this thread moves every K step (the K step only shifts the channel offset).  Rows and columns past the
    // image, output channels past ldy and channels past C are staged as zeros (C % CHK == 0: a chunk is all in or all out)
    constexpr int XPT = (DC_XCHUNKS + DC_THREADS - 1) / DC_THREADS, WPT = (WCHUNKS + DC_THREADS - 1) / DC_THREADS;
    unsigned xoff[XPT], woff[WPT];                       // byte offset of the chunk at K step 0; 0xffffffff: always zero (host: both tensors < 2 GiB)
#pragma unroll
    for (int k = 0; k < XPT; ++k) {
        const int id = tid + k * DC_THREADS, c = id & 3, hp = id >> 2, r = hp / DC_HW, col = hp - r * DC_HW;
        const int ih = i0 + r, iw = j0 + col;
        xoff[k] = (id < DC_XCHUNKS && ih < p.H && iw < p.W) ? (unsigned)((((n * p.H + ih) * p.W + iw) * p.C + c * CHK) * ES) : 0xffffffffu;
    }
#pragma unroll
    for (int k = 0; k < WPT; ++k) {
        const int id = tid + k * DC_THREADS, c = id & 3, q = id >> 2, co = q % NCO, tap = q / NCO, row = co0 + co;
        woff[k] = (id < WCHUNKS && row < p.ldy) ? (unsigned)(((row * 9 + tap) * p.C + c * CHK) * ES) : 0xffffffffu;
    }
    uint4 rx[XPT], rw[WPT];
    auto load_step = [&](int s) {                        // global -> registers: issued one K step ahead, underneath the MFMAs of the running step
        const int chb = s * KSTEP, cl = chb + (tid & 3) * CHK;       // (id & 3 == tid & 3 for every chunk of this thread)
#pragma unroll
        for (int k = 0; k < XPT; ++k)
            rx[k] = (xoff[k] != 0xffffffffu && cl < p.C) ? *reinterpret_cast<const uint4*>(xg + xoff[k] + chb * ES) : uint4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < WPT; ++k)
            rw[k] = (woff[k] != 0xffffffffu && cl < p.C) ? *reinterpret_cast<const uint4*>(wg + woff[k] + chb * ES) : uint4{0u, 0u, 0u, 0u};
    };

    const int ksteps = (p.C + KSTEP - 1) / KSTEP;
    load_step(0);
    for (int s = 0; s < ksteps; ++s) {
        __syncthreads();                                 // every wave is done with the previous K step's tiles
#pragma unroll
        for (int k = 0; k < XPT; ++k)
            if (tid + k * DC_THREADS < DC_XCHUNKS) *reinterpret_cast<uint4*>(sX + (tid + k * DC_THREADS) * 16) = rx[k];
#pragma unroll
        for (int k = 0; k < WPT; ++k)
            if (tid + k * DC_THREADS < WCHUNKS) *reinterpret_cast<uint4*>(sW + (tid + k * DC_THREADS) * 16) = rw[k];
        __syncthreads();
        if (s + 1 < ksteps) load_step(s + 1);
        // ---- wave -> tile rows 2 wave, 2 wave + 1 (halo rows 2 wave .. 2 wave + 2); lane = (pixel li, K chunk lg)
        const unsigned char* xb = sX + (((2 * wave) * DC_HW + li) * 4 + lg) * 16;
        uint4 b[3][2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) b[r][dx] = *reinterpret_cast<const uint4*>(xb + (r * DC_HW + dx) * 64);
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ty = tap / 3, tx = tap - ty * 3;
                const int q = (ty != 1 ? 2 : 0) + (tx != 1 ? 1 : 0), dy = ty == 2 ? 1 : 0, dx = tx == 2 ? 1 : 0;
                const uint4 a = *reinterpret_cast<const uint4*>(sW + (((tap * NCO + cb * 16 + li) * 4 + lg) * 16));
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) acc[rr][q][cb] = DcT<T>::mma(a, b[rr + dy][dx], acc[rr][q][cb]);
            }
    }

    // ---- epilogue: lane = (input pixel column j0 + li, output channels 4 lg .. 4 lg + 3 of every 16-channel block)
    const int j = j0 + li;
    if (j >= p.W) return;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int co = co0 + cb * 16 + 4 * lg;
        if (co >= p.ldy) continue;                       // ldy % 4 == 0: a lane's four channels are all inside or all outside
        float bias4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bias4[e] = (p.bias && co + e < p.Cout) ? p.bias[co + e] : 0.f;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int i = i0 + 2 * wave + rr;
            if (i >= p.H) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int oh = 2 * i + (q >> 1), ow = 2 * j + (q & 1);
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float z = acc[rr][q][cb][e] + bias4[e];
                    if (p.act == SDE_ACT_RELU) z = z > 0.f ? z : 0.f;
                    else if (p.act == SDE_ACT_ELU) z = z > 0.f ? z : expm1f(z);
                    v[e] = co + e < p.Cout ? z : 0.f;
                }
                unsigned char* dst = static_cast<unsigned char*>(p.y) + ((((size_t)n * 2 * p.H + oh) * 2 * p.W + ow) * p.ldy + co) * ES;
                DcT<T>::store4(dst, v);
            }
        }
    }
}

template <typename T>
void deconv_launch(const DeconvP& p, hipStream_t s) {
    const int tiles = p.B * p.tiles_h * p.tiles_w;
    if (p.ldy > 16) hipLaunchKernelGGL((deconv3x3s2_kernel<T, 2>), dim3(tiles, sde_cdiv(p.ldy, 32)), dim3(DC_THREADS), 0, s, p);
    else hipLaunchKernelGGL((deconv3x3s2_kernel<T, 1>), dim3(tiles, 1), dim3(DC_THREADS), 0, s, p);
}

}  // namespace

extern "C" int sde_deconv3x3s2_fwd(const void* x, const void* w_packed, const float* bias, int act, int B, int H, int W, int C, int Cout, int ldy, int dtype,
                                   void* y, sde_stream_t stream) {
    SDE_CHECK_ARG(x && w_packed && y, "sde_deconv3x3s2_fwd: null pointer");
    SDE_CHECK_ARG(dtype == SDE_F32 || dtype == SDE_BF16, "sde_deconv3x3s2_fwd: fp32 or bf16 storage only (dtype %d)", dtype);
    const int V = dtype == SDE_F32 ? 4 : 8;
    SDE_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % V == 0, "sde_deconv3x3s2_fwd: bad input shape [%d,%d,%d,%d]", B, H, W, C);
    SDE_CHECK_ARG(Cout > 0 && ldy >= Cout && ldy % V == 0, "sde_deconv3x3s2_fwd: bad Cout=%d ldy=%d", Cout, ldy);
    SDE_CHECK_ARG(act == SDE_ACT_NONE || act == SDE_ACT_ELU || act == SDE_ACT_RELU, "sde_deconv3x3s2_fwd: bad act %d", act);
    SDE_CHECK_ARG(4L * B * H * W <= 0x7fffffffL, "sde_deconv3x3s2_fwd: too many output pixels");
    const long es = dtype == SDE_F32 ? 4 : 2;
    SDE_CHECK_ARG((long)B * H * W * C * es < 0x7fffffffL && 9L * ldy * C * es < 0x7fffffffL, "sde_deconv3x3s2_fwd: input and operand must be below 2 GiB");
    DeconvP p;
    p.x = x; p.w = w_packed; p.bias = bias; p.y = y;
    p.B = B; p.H = H; p.W = W; p.C = C; p.Cout = Cout; p.ldy = ldy; p.act = act;
    p.tiles_h = sde_cdiv(H, DC_TH); p.tiles_w = sde_cdiv(W, DC_TW);
    SDE_CHECK_ARG((long)B * p.tiles_h * p.tiles_w <= 0x7fffffffL && sde_cdiv(ldy, 32) <= 65535, "sde_deconv3x3s2_fwd: grid too large");
    if (dtype == SDE_BF16) deconv_launch<bf16_t>(p, (hipStream_t)stream); else deconv_launch<float>(p, (hipStream_t)stream);
    SDE_CHECK_LAUNCH("sde_deconv3x3s2_fwd");
    return SDE_OK;
}
