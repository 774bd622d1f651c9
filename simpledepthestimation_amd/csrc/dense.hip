// DenseNet dense blocks without the concatenation (torchvision densenet.py _DenseLayer / _Transition, under BTSNet.py:L283-290).
//
// A dense block is kept as its PIECES: the block input [M,C0] and one [M,g] tensor per layer, each the plain NHWC output of the layer's 3x3
// convolution.  torch's layer l computes relu(norm1(cat(pieces[:l]))): the concatenation copies the whole growing map and the BatchNorm reduces
// it again, although a channel's statistics are fixed once its producer has written it.  Here
//
//   dense_stats            one small launch per NEW piece turns the producing convolution's (sum, sum^2) slab into (mean, biased variance) rows of
//                          the block's table [Ct][2]; later layers only read them
//   dense_bn_relu_fwd      gathers the pieces through a by-value pointer table, normalises with the table and the layer's gamma / beta, ReLU, and
//                          writes the contiguous [M,Cin] operand of the 1x1 convolution (one read of the pieces, one write)
//   dense_bn_relu_bwd      reduce launch (sum gm, sum gm * xhat per channel; the ReLU mask is re-derived from the pieces) + apply launch, which first
//                          sums the partial rows of its own 64 channels, then writes dx [M,Cin]
//   dense_grad_gather      gradient of piece j = [outside gradient +] the column slices [off_j, off_j + g) of every later layer's dx, summed in
//                          fp32 in a fixed order: one launch per piece instead of one autograd add per consumer
//   avgpool2x2             AvgPool2d(2, 2) of the transitions (odd sizes floor)
//
// A workgroup owns up to 8 sixteen-byte channel groups (64 bf16 / 32 fp32 channels) of a range of rows: a lane keeps its channel group for the
// whole launch, so the piece it reads is looked up once.  No atomics, every sum has one order: two runs give the same bits.
#include "vec16.h"
#include "launch.h"

namespace {

struct DenseTab {
    const void* p[SDE_DENSE_MAX];
    int off[SDE_DENSE_MAX + 1];      // first channel of every piece; off[n] = Cin
    int n;
};

struct GatherTab {
    const void* p[SDE_DENSE_MAX];
    int ld[SDE_DENSE_MAX];
    int n;
};

constexpr int DCW = 8;               // sixteen-byte channel groups per workgroup
constexpr int DENSE_ROWS = 64;       // most partial rows of the backward reduction

// the lane's place: channel group cv (of cch), row lane rl (of rp); lanes beyond rp * cw or beyond the last channel group idle
struct Lane { int cw, rp, cl, rl, cv; bool on; };
__device__ __forceinline__ Lane lane_of(int cch) {
    Lane l;
    l.cw = cch < DCW ? cch : DCW;
    l.rp = 256 / l.cw;
    l.cl = threadIdx.x % l.cw;
    l.rl = threadIdx.x / l.cw;
    l.cv = blockIdx.y * l.cw + l.cl;
    l.on = l.rl < l.rp && l.cv < cch;
    return l;
}

// piece holding channel c0 (wave-uniform loop over the kernel argument: scalar loads)
template <typename T>
__device__ __forceinline__ void find_piece(const DenseTab& t, int c0, const T*& src, int& width, int& coff) {
    src = nullptr; width = 0; coff = 0;
    for (int k = 0; k < t.n; ++k)
        if (c0 >= t.off[k] && c0 < t.off[k + 1]) {
            src = reinterpret_cast<const T*>(t.p[k]);
            width = t.off[k + 1] - t.off[k];
            coff = c0 - t.off[k];
        }
}

// (sum, sum^2) slab [rows][C][2] of one piece -> table rows (mean, biased variance); 8 channels per workgroup, 16 row lanes, double sums
__global__ void __launch_bounds__(256) dense_stats_kernel(const float* __restrict__ slab, int rows, int C, double count, float* __restrict__ table) {
    __shared__ double sh[256];
    const int e = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int col = blockIdx.x * 16 + e;
    double a = 0;
    if (col < 2 * C)
        for (int r = rl; r < rows; r += 16) a += (double)slab[(size_t)r * 2 * C + col];
    sh[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x < 16) {
        double tot = 0;
        for (int i = 0; i < 16; ++i) tot += sh[i * 16 + threadIdx.x];
        sh[threadIdx.x] = tot;
    }
    __syncthreads();
    const int c = blockIdx.x * 8 + threadIdx.x;
    if (threadIdx.x < 8 && c < C) {
        const double mean = sh[2 * threadIdx.x] / count;
        double var = sh[2 * threadIdx.x + 1] / count - mean * mean;
        if (var < 0) var = 0;
        table[2 * c] = (float)mean;
        table[2 * c + 1] = (float)var;
    }
}

// bnp [4][C] = mean, rstd, scale, shift from the table (training; running statistics updated as torch does) or from the running statistics (table == null)
__global__ void __launch_bounds__(256) dense_params_kernel(const float* __restrict__ table, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ rmean, float* __restrict__ rvar, float momentum, float eps, float count, int C,
                                                           float* __restrict__ bnp) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float mean, var;
    if (table) {
        mean = table[2 * c]; var = table[2 * c + 1];
        if (rmean) {
            const double unb = count > 1.f ? (double)var * count / (count - 1.0) : (double)var;
            rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
            rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unb;
        }
    } else {
        mean = rmean[c]; var = rvar[c];
    }
    const float rstd = (float)(1.0 / sqrt((double)var + (double)eps));
    const float sc = gamma[c] * rstd;
    bnp[c] = mean; bnp[C + c] = rstd; bnp[2 * C + c] = sc; bnp[3 * C + c] = beta[c] - mean * sc;
}

template <typename T>
__global__ void __launch_bounds__(256) dense_fwd_kernel(const DenseTab t, long M, int Cin, const float* __restrict__ bnp, T* __restrict__ out, long rpb) {
    constexpr int V = VecOf<T>::V;
    const Lane l = lane_of(Cin / V);
    if (!l.on) return;
    const int c0 = l.cv * V;
    const T* src; int width, coff;
    find_piece<T>(t, c0, src, width, coff);
    float sc[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { sc[j] = bnp[2 * Cin + c0 + j]; sh[j] = bnp[3 * Cin + c0 + j]; }
    const long r0 = (long)blockIdx.x * rpb;
    const long r1 = r0 + rpb < M ? r0 + rpb : M;
    for (long m = r0 + l.rl; m < r1; m += l.rp) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + m * width + coff);
        const T* x = reinterpret_cast<const T*>(&v);
        T o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (T)fmaxf(fmaf((float)x[j], sc[j], sh[j]), 0.f);
        *reinterpret_cast<uint4*>(out + m * Cin + c0) = *reinterpret_cast<const uint4*>(o);
    }
}

// part [gridDim.x][Cin][2] = per-workgroup (sum gm, sum gm * xhat), gm = g * [scale * x + shift > 0]
template <typename T>
__global__ void __launch_bounds__(256) dense_bwd_reduce_kernel(const DenseTab t, long M, int Cin, const T* __restrict__ g, const float* __restrict__ bnp,
                                                               float* __restrict__ part, long rpb) {
    constexpr int V = VecOf<T>::V;
    __shared__ float sh[256 * 2 * V];
    const int cch = Cin / V;
    const Lane l = lane_of(cch);
    float s0[V], s1[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s0[j] = s1[j] = 0.f;
    if (l.on) {
        const int c0 = l.cv * V;
        const T* src; int width, coff;
        find_piece<T>(t, c0, src, width, coff);
        float mean[V], rstd[V], sc[V], sf[V];
#pragma unroll
        for (int j = 0; j < V; ++j) { mean[j] = bnp[c0 + j]; rstd[j] = bnp[Cin + c0 + j]; sc[j] = bnp[2 * Cin + c0 + j]; sf[j] = bnp[3 * Cin + c0 + j]; }
        const long r0 = (long)blockIdx.x * rpb;
        const long r1 = r0 + rpb < M ? r0 + rpb : M;
        for (long m = r0 + l.rl; m < r1; m += l.rp) {
            const uint4 vx = *reinterpret_cast<const uint4*>(src + m * width + coff);
            const uint4 vg = *reinterpret_cast<const uint4*>(g + m * Cin + c0);
            const T* x = reinterpret_cast<const T*>(&vx);
            const T* gg = reinterpret_cast<const T*>(&vg);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float xf = (float)x[j];
                const float gm = fmaf(xf, sc[j], sf[j]) > 0.f ? (float)gg[j] : 0.f;
                s0[j] += gm;
                s1[j] = fmaf(gm, (xf - mean[j]) * rstd[j], s1[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) { sh[threadIdx.x * 2 * V + 2 * j] = s0[j]; sh[threadIdx.x * 2 * V + 2 * j + 1] = s1[j]; }
    __syncthreads();
    if ((int)threadIdx.x < l.cw * 2 * V) {
        const int cl2 = threadIdx.x / (2 * V), e = threadIdx.x % (2 * V);
        const int cv2 = blockIdx.y * l.cw + cl2;
        float tot = 0.f;
        for (int r = 0; r < l.rp; ++r) tot += sh[(r * l.cw + cl2) * 2 * V + e];
        if (cv2 < cch) part[(size_t)blockIdx.x * 2 * Cin + (size_t)cv2 * V * 2 + e] = tot;
    }
}

// dx = scale * (gm - mean(gm) - xhat * mean(gm * xhat)); the workgroups of row range 0 also write dgamma / dbeta (either may be null)
template <typename T>
__global__ void __launch_bounds__(256) dense_bwd_apply_kernel(const DenseTab t, long M, int Cin, const T* __restrict__ g, const float* __restrict__ bnp,
                                                              const float* __restrict__ part, int R, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              int accumulate, T* __restrict__ dx, long rpb) {
    constexpr int V = VecOf<T>::V;
    __shared__ float coef[DCW * 2 * V];
    const int cch = Cin / V;
    const Lane l = lane_of(cch);
    if ((int)threadIdx.x < l.cw * 2 * V) {
        const int cl2 = threadIdx.x / (2 * V), e = threadIdx.x % (2 * V);
        const int cv2 = blockIdx.y * l.cw + cl2;
        float tot = 0.f;
        if (cv2 < cch) {
            for (int r = 0; r < R; ++r) tot += part[(size_t)r * 2 * Cin + (size_t)cv2 * V * 2 + e];
            if (blockIdx.x == 0) {
                float* dst = (e & 1) ? dgamma : dbeta;
                const int c = cv2 * V + (e >> 1);
                if (dst) dst[c] = accumulate ? dst[c] + tot : tot;
            }
        }
        coef[threadIdx.x] = tot / (float)M;
    }
    __syncthreads();
    if (!l.on) return;
    const int c0 = l.cv * V;
    const T* src; int width, coff;
    find_piece<T>(t, c0, src, width, coff);
    float mean[V], rstd[V], sc[V], sf[V], k1[V], k2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        mean[j] = bnp[c0 + j]; rstd[j] = bnp[Cin + c0 + j]; sc[j] = bnp[2 * Cin + c0 + j]; sf[j] = bnp[3 * Cin + c0 + j];
        k1[j] = coef[l.cl * 2 * V + 2 * j]; k2[j] = coef[l.cl * 2 * V + 2 * j + 1];
    }
    const long r0 = (long)blockIdx.x * rpb;
    const long r1 = r0 + rpb < M ? r0 + rpb : M;
    for (long m = r0 + l.rl; m < r1; m += l.rp) {
        const uint4 vx = *reinterpret_cast<const uint4*>(src + m * width + coff);
        const uint4 vg = *reinterpret_cast<const uint4*>(g + m * Cin + c0);
        const T* x = reinterpret_cast<const T*>(&vx);
        const T* gg = reinterpret_cast<const T*>(&vg);
        T o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float xf = (float)x[j];
            const float gm = fmaf(xf, sc[j], sf[j]) > 0.f ? (float)gg[j] : 0.f;
            o[j] = (T)(sc[j] * (gm - k1[j] - (xf - mean[j]) * rstd[j] * k2[j]));
        }
        *reinterpret_cast<uint4*>(dx + m * Cin + c0) = *reinterpret_cast<const uint4*>(o);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) dense_gather_kernel(const GatherTab t, long M, int off, int g, const T* __restrict__ outside, T* __restrict__ out) {
    constexpr int V = VecOf<T>::V;
    const int cg = g / V;
    const long total = M * cg;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int gv = (int)(i % cg);
        const long m = i / cg;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        if (outside) {
            const uint4 v = *reinterpret_cast<const uint4*>(outside + m * g + gv * V);
            const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = (float)e[j];
        }
        for (int k = 0; k < t.n; ++k) {
            const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(t.p[k]) + m * t.ld[k] + off + gv * V);
            const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] += (float)e[j];
        }
        T o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (T)acc[j];
        *reinterpret_cast<uint4*>(out + m * g + gv * V) = *reinterpret_cast<const uint4*>(o);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) avgpool2_fwd_kernel(const T* __restrict__ x, T* __restrict__ out, int B, int H, int W, int C) {
    constexpr int V = VecOf<T>::V;
    const int cg = C / V, OH = H / 2, OW = W / 2;
    const long total = (long)B * OH * OW * cg;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int gv = (int)(i % cg);
        const long pix = i / cg;
        const int ox = (int)(pix % OW), oy = (int)((pix / OW) % OH), b = (int)(pix / ((long)OW * OH));
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = *reinterpret_cast<const uint4*>(x + (((long)b * H + 2 * oy + (k >> 1)) * W + 2 * ox + (k & 1)) * C + gv * V);
            const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] += (float)e[j];
        }
        T o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (T)(acc[j] * 0.25f);
        *reinterpret_cast<uint4*>(out + pix * C + gv * V) = *reinterpret_cast<const uint4*>(o);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) avgpool2_bwd_kernel(const T* __restrict__ dout, T* __restrict__ dx, int B, int H, int W, int C) {
    constexpr int V = VecOf<T>::V;
    const int cg = C / V, OH = H / 2, OW = W / 2;
    const long total = (long)B * H * W * cg;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int gv = (int)(i % cg);
        const long pix = i / cg;
        const int xx = (int)(pix % W), yy = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
        T o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (T)0.f;
        if ((yy >> 1) < OH && (xx >> 1) < OW) {       // the odd last row / column is outside every window
            const uint4 v = *reinterpret_cast<const uint4*>(dout + (((long)b * OH + (yy >> 1)) * OW + (xx >> 1)) * C + gv * V);
            const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = (T)((float)e[j] * 0.25f);
        }
        *reinterpret_cast<uint4*>(dx + pix * C + gv * V) = *reinterpret_cast<const uint4*>(o);
    }
}

typedef SdeTypes<bf16_t, float> Types;
constexpr int GRID_CAP = SDE_GRID_CAP_16K;

int build_tab(const sde_dense_desc* d, int dtype, DenseTab& t, const char* who) {
    SDE_CHECK_ARG(d, "%s: null descriptor", who);
    SDE_CHECK_ARG(Types::has(dtype), "%s: fp32 and bf16 only (dtype %d)", who, dtype);
    SDE_CHECK_ARG(d->n >= 1 && d->n <= SDE_DENSE_MAX, "%s: 1..%d pieces, got %d", who, SDE_DENSE_MAX, d->n);
    t.n = d->n;
    t.off[0] = 0;
    for (int k = 0; k < d->n; ++k) {
        SDE_CHECK_ARG(d->p[k] && d->C[k] > 0 && d->C[k] % 8 == 0, "%s: piece %d needs a pointer and a width that is a multiple of 8 (C=%d)", who, k, d->C[k]);
        t.p[k] = d->p[k];
        t.off[k + 1] = t.off[k] + d->C[k];
    }
    for (int k = d->n; k < SDE_DENSE_MAX; ++k) { t.p[k] = nullptr; t.off[k + 1] = t.off[d->n]; }
    return SDE_OK;
}

// rows a lane pass covers, channel-group columns of the grid
void dense_geometry(int Cin, int dtype, int& rp, int& ny) {
    const int V = sde_vec_elems(dtype);
    const int cch = Cin / V;
    const int cw = cch < DCW ? cch : DCW;
    rp = 256 / cw;
    ny = (cch + cw - 1) / cw;
}

long row_blocks(long M, int rp, long cap) {
    long nb = (M + rp - 1) / rp;
    if (nb > cap) nb = cap;
    return nb < 1 ? 1 : nb;
}

}  // namespace

extern "C" {

int sde_dense_stats(const float* slab, int rows, int C, long count, float* table, int off, sde_stream_t stream) {
    SDE_CHECK_ARG(slab && table && rows > 0 && C > 0 && C % 8 == 0 && count > 0 && off >= 0 && off % 8 == 0, "sde_dense_stats: bad argument (rows=%d C=%d off=%d)", rows,
                  C, off);
    hipLaunchKernelGGL(dense_stats_kernel, dim3(sde_cdiv(C, 8)), dim3(256), 0, (hipStream_t)stream, slab, rows, C, (double)count, table + 2 * (size_t)off);
    SDE_CHECK_LAUNCH("sde_dense_stats");
    return SDE_OK;
}

int sde_dense_bwd_rows(long M, int Cin, int dtype) {
    SDE_CHECK_ARG(Types::has(dtype), "sde_dense_bwd_rows: fp32 and bf16 only (dtype %d)", dtype);
    SDE_CHECK_ARG(M > 0 && Cin > 0 && Cin % 8 == 0, "sde_dense_bwd_rows: M > 0 and a channel count that is a multiple of 8 (M=%ld Cin=%d)", M, Cin);
    int rp, ny;
    dense_geometry(Cin, dtype, rp, ny);
    return (int)row_blocks(M, rp, DENSE_ROWS);
}

int sde_dense_bn_relu_fwd(const sde_dense_desc* d, long M, int dtype, const float* table, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, float* bnp, void* out, sde_stream_t stream) {
    DenseTab t;
    const int rc = build_tab(d, dtype, t, "sde_dense_bn_relu_fwd");
    if (rc) return rc;
    SDE_CHECK_ARG(M > 0 && gamma && beta && bnp && out, "sde_dense_bn_relu_fwd: bad argument");
    SDE_CHECK_ARG(table || (running_mean && running_var), "sde_dense_bn_relu_fwd: eval mode (no table) needs the running statistics");
    SDE_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "sde_dense_bn_relu_fwd: running_mean and running_var go together");
    const int Cin = t.off[t.n];
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dense_params_kernel, dim3(sde_cdiv(Cin, 256)), dim3(256), 0, s, table, gamma, beta, running_mean, running_var, momentum, eps, (float)M, Cin, bnp);
    SDE_CHECK_LAUNCH("sde_dense_bn_relu_fwd/params");
    int rp, ny;
    dense_geometry(Cin, dtype, rp, ny);
    const long nx = row_blocks(M, rp, 1024);
    const long rpb = (M + nx - 1) / nx;
    const dim3 grid((unsigned)nx, (unsigned)ny);
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(dense_fwd_kernel<T>, grid, dim3(256), 0, s, t, M, Cin, bnp, (T*)out, rpb);
    });
    SDE_CHECK_LAUNCH("sde_dense_bn_relu_fwd");
    return SDE_OK;
}

int sde_dense_bn_relu_bwd(const sde_dense_desc* d, long M, int dtype, const void* g, const float* bnp, float* part, float* dgamma, float* dbeta,
                          int accumulate_params, void* dx, sde_stream_t stream) {
    DenseTab t;
    const int rc = build_tab(d, dtype, t, "sde_dense_bn_relu_bwd");
    if (rc) return rc;
    SDE_CHECK_ARG(M > 0 && g && bnp && part && dx, "sde_dense_bn_relu_bwd: bad argument");
    const int Cin = t.off[t.n];
    int rp, ny;
    dense_geometry(Cin, dtype, rp, ny);
    const int R = (int)row_blocks(M, rp, DENSE_ROWS);
    const long rpb = (M + R - 1) / R;
    const long nx = row_blocks(M, rp, 256);
    const long rpa = (M + nx - 1) / nx;
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(dense_bwd_reduce_kernel<T>, dim3(R, ny), dim3(256), 0, s, t, M, Cin, (const T*)g, bnp, part, rpb);
        hipLaunchKernelGGL(dense_bwd_apply_kernel<T>, dim3((unsigned)nx, ny), dim3(256), 0, s, t, M, Cin, (const T*)g, bnp, part, R, dgamma, dbeta, accumulate_params,
                           (T*)dx, rpa);
    });
    SDE_CHECK_LAUNCH("sde_dense_bn_relu_bwd");
    return SDE_OK;
}

int sde_dense_grad_gather(const sde_dense_desc* dxs, long M, int off, int g, int dtype, const void* outside, void* out, sde_stream_t stream) {
    SDE_CHECK_ARG(dxs && out, "sde_dense_grad_gather: null pointer");
    SDE_CHECK_ARG(Types::has(dtype), "sde_dense_grad_gather: fp32 and bf16 only (dtype %d)", dtype);
    SDE_CHECK_ARG(dxs->n >= 0 && dxs->n <= SDE_DENSE_MAX && (dxs->n > 0 || outside), "sde_dense_grad_gather: 0..%d sources (none only with an outside gradient), got %d",
                  SDE_DENSE_MAX, dxs->n);
    SDE_CHECK_ARG(M > 0 && off >= 0 && off % 8 == 0 && g > 0 && g % 8 == 0, "sde_dense_grad_gather: offset and width must be multiples of 8 (off=%d g=%d)", off, g);
    GatherTab t;
    t.n = dxs->n;
    for (int k = 0; k < SDE_DENSE_MAX; ++k) {
        if (k < dxs->n) SDE_CHECK_ARG(dxs->p[k] && dxs->C[k] % 8 == 0 && off + g <= dxs->C[k], "sde_dense_grad_gather: source %d (width %d) does not hold columns [%d, %d)",
                                      k, dxs->C[k], off, off + g);
        t.p[k] = k < dxs->n ? dxs->p[k] : nullptr;
        t.ld[k] = k < dxs->n ? dxs->C[k] : 0;
    }
    const int V = sde_vec_elems(dtype);
    const int nb = sde_grid_for(M * (g / V), GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(dense_gather_kernel<T>, dim3(nb), dim3(256), 0, s, t, M, off, g, (const T*)outside, (T*)out);
    });
    SDE_CHECK_LAUNCH("sde_dense_grad_gather");
    return SDE_OK;
}

int sde_avgpool2x2_fwd(const void* x, int B, int H, int W, int C, int dtype, void* out, sde_stream_t stream) {
    SDE_CHECK_ARG(Types::has(dtype), "sde_avgpool2x2_fwd: fp32 and bf16 only (dtype %d)", dtype);
    SDE_CHECK_ARG(x && out && B > 0 && H >= 2 && W >= 2 && C > 0 && C % 8 == 0, "sde_avgpool2x2_fwd: bad argument (H=%d W=%d C=%d)", H, W, C);
    const int V = sde_vec_elems(dtype);
    const int nb = sde_grid_for((long)B * (H / 2) * (W / 2) * (C / V), GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(avgpool2_fwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)x, (T*)out, B, H, W, C);
    });
    SDE_CHECK_LAUNCH("sde_avgpool2x2_fwd");
    return SDE_OK;
}

int sde_avgpool2x2_bwd(const void* dout, int B, int H, int W, int C, int dtype, void* dx, sde_stream_t stream) {
    SDE_CHECK_ARG(Types::has(dtype), "sde_avgpool2x2_bwd: fp32 and bf16 only (dtype %d)", dtype);
    SDE_CHECK_ARG(dout && dx && B > 0 && H >= 2 && W >= 2 && C > 0 && C % 8 == 0, "sde_avgpool2x2_bwd: bad argument (H=%d W=%d C=%d)", H, W, C);
    const int V = sde_vec_elems(dtype);
    const int nb = sde_grid_for((long)B * H * W * (C / V), GRID_CAP);
    hipStream_t s = (hipStream_t)stream;
    Types::dispatch(dtype, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(avgpool2_bwd_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)dout, (T*)dx, B, H, W, C);
    });
    SDE_CHECK_LAUNCH("sde_avgpool2x2_bwd");
    return SDE_OK;
}

}  // extern "C"
