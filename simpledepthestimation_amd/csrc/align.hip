// Frame-to-model alignment: the camera tracked against the TSDF volume.  One call of sde_frame_align is ONE Gauss-Newton iteration of a
// point-to-plane fit of the current frame's depth to the model rendered by sde_tsdf_render, plus the update of a depth scale.  The contract is
// written out in include/sde_hip.h.
//
// align_reset        state <- D = Dinv = I, s = 1, info = 0: one workgroup of 64 threads.
// align_accumulate   one pixel per thread, sde_tsdf_render's tile (a wave is 8 x 8 pixels, a workgroup four of them side by side): the pixel is
//                    lifted with the scale, moved by D, projected onto the rendered model, and gives 31 fp32 terms (21 J_i J_j, 6 J_i r, r^2,
//                    count, rho, scale count; 0 where it is not kept).  sde_block_sums adds them over the workgroup; threads 0..31 write the
//                    workgroup's row of the slab.  Every workgroup writes its whole row: the workspace needs no clearing.  Per pixel 4 B of depth
//                    and, where the point lands on the picture, 16 B of the model are read; the state's 13 words are uniform.
// align_finish       ONE workgroup of 1024 threads = 32 row groups x 32 columns sums the slab in fp64 (thread (g, k) adds column k of the rows
//                    g, g + 32, ... in ascending order; column k's 32 group sums are added as a balanced binary tree), then thread 0 solves the
//                    damped normal equations by LDL^T in fp64, forms the Cayley rotation in fp64, and composes D, Dinv and s in fp32.
// No atomics, no ticket, no workgroup that waits for another; nothing is written but the state and the workspace.
//
// Built with -ffp-contract=off: the per-pixel stage, the solve and the update keep the operation order the header states, which hip/align.py's
// host twins repeat bit for bit.
#include "common.h"
#include "pinhole.h"
#include "sde_hip.h"

namespace {

constexpr int TW = 32, TH = 8;                   // pixels per workgroup: four 8 x 8 waves side by side (sde_tsdf_render's tile)
constexpr int NV = SDE_ALIGN_SUMS;               // 31 sums, padded to 32
constexpr int MAX_PICTURE = 32768;
constexpr int FIN_THREADS = 1024, FIN_GROUPS = FIN_THREADS / NV;

struct AccumP {
    const float* pred;           // [ph][pw]
    const int* ymap;             // [H]
    const int* xmap;             // [W]
    const float* K;              // [3][3]
    const float* depth;          // [H][W] the model's z-depth
    const float* normal;         // [H][W][3]
    const float* state;
    float* slab;                 // [blocks][NV]
    int H, W, ph, pw;
    float min_depth, max_depth, dist_tol, scale_tol;
};

__global__ void __launch_bounds__(64) align_reset(float* state) {
    const int t = threadIdx.x;
    if (t >= SDE_ALIGN_STATE_WORDS) return;
    float v = 0.f;
    if (t < 32) v = ((t & 15) % 5 == 0) ? 1.f : 0.f;                                     // D and Dinv: the identity
    else if (t == SDE_ALIGN_SCALE_AT) v = 1.f;
    state[t] = v;                                                                        // the info words: all bits zero
}

__global__ void __launch_bounds__(TW * TH) align_accumulate(AccumP p) {
    __shared__ float red[(TW * TH / 64) * NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * TW + wave * 8 + (lane & 7), v = blockIdx.y * TH + (lane >> 3);
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    do {                                                                                 // one pass; `break` = the pixel is not kept
        if (u >= p.W || v >= p.H) break;
        const int my = p.ymap[v], mx = p.xmap[u];
        if (my < 0 || mx < 0) break;
        const float d0 = p.pred[(size_t)my * p.pw + mx];
        if (!(fabsf(d0) < INFINITY && p.min_depth < d0 && d0 <= p.max_depth)) break;
        const float d = p.state[SDE_ALIGN_SCALE_AT] * d0;
        const Pinhole cam = pinhole_load(p.K);
        const float rx = cam.k00 * (float)u + cam.k02, ry = cam.k11 * (float)v + cam.k12;
        const float px = d * rx, py = d * ry;
        float qx, qy, qz, X, Y;
        pinhole_move<4>(p.state, px, py, d, p.state[3], p.state[7], p.state[11], qx, qy, qz);
        if (!(qz > 0.f && qz < INFINITY)) break;                                         // a NaN fails the comparison
        pinhole_project(cam, qx, qy, qz, X, Y);
        int ix, iy;
        if (!nearest_pixel(X, Y, ix, iy)) break;
        if (ix < 0 || ix >= p.W || iy < 0 || iy >= p.H) break;
        const size_t at = (size_t)iy * p.W + ix;
        const float m = p.depth[at];
        if (!(m > 0.f)) break;
        const float nx = p.normal[3 * at], ny = p.normal[3 * at + 1], nz = p.normal[3 * at + 2];
        if (nx == 0.f && ny == 0.f && nz == 0.f) break;
        const float gx = m * (cam.k00 * (float)ix + cam.k02), gy = m * (cam.k11 * (float)iy + cam.k12);
        const float ex = qx - gx, ey = qy - gy, ez = qz - m;
        const float r = nx * ex + ny * ey + nz * ez;
        if (fabsf(r) <= p.dist_tol * m) {                                                // a NaN fails the comparison
            const float J[6] = {qy * nz - qz * ny, qz * nx - qx * nz, qx * ny - qy * nx, nx, ny, nz};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) acc[k++] = J[i] * J[j];
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[21 + i] = J[i] * r;
            acc[27] = r * r;
            acc[28] = 1.f;
        }
        const float rho = m / qz;
        if (fabsf(rho - 1.f) <= p.scale_tol) {
            acc[29] = rho;
            acc[30] = 1.f;
        }
    } while (false);
    sde_block_sums<NV, TW * TH / 64>(acc, red, p.slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NV);
}

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) < (double)INFINITY; }

__global__ void __launch_bounds__(FIN_THREADS) align_finish(const float* __restrict__ slab, int rows, int min_count, float damping, int mode, float* state) {
    __shared__ double part[FIN_GROUPS][NV];
    __shared__ double total[NV];
    const int k = threadIdx.x & (NV - 1), g = threadIdx.x / NV;
    double a = 0.0;
    for (int i = g; i < rows; i += FIN_GROUPS) a += (double)slab[(size_t)i * NV + k];
    part[g][k] = a;
    __syncthreads();
    if (threadIdx.x < NV) {
        double t[FIN_GROUPS];
#pragma unroll
        for (int i = 0; i < FIN_GROUPS; ++i) t[i] = part[i][k];
#pragma unroll
        for (int n = FIN_GROUPS; n > 1; n >>= 1)                                         // (t0 + t1), (t2 + t3), ...: a balanced binary tree
#pragma unroll
            for (int i = 0; i < n / 2; ++i) t[i] = t[2 * i] + t[2 * i + 1];
        total[k] = t[0];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;

    int* info = (int*)state;
    const int count = (int)total[28], count_s = (int)total[30];                          // sums of 0 / 1: exact integers, at most 2^30
    info[SDE_ALIGN_COUNT_AT] = count;
    info[SDE_ALIGN_SCALE_COUNT_AT] = count_s;
    state[SDE_ALIGN_SUMSQ_AT] = (float)total[27];
    if (count < min_count) { info[SDE_ALIGN_STATUS_AT] = SDE_ALIGN_TOO_FEW; return; }

    float Dn[12];
    if (mode & SDE_ALIGN_POSE) {
        double A[6][6], L[6][6], dg[6], x[6];
        int at = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = total[at++];
        const double lm = 1.0 + (double)damping;
        for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] * lm;
        bool ok = true;
        for (int j = 0; j < 6 && ok; ++j) {                                              // A = L diag(dg) L^T, no pivoting
            double s = A[j][j];
            for (int c = 0; c < j; ++c) s = s - (L[j][c] * L[j][c]) * dg[c];
            dg[j] = s;
            ok = s > 0.0 && finite_d(s);
            for (int i = j + 1; i < 6 && ok; ++i) {
                double w = A[i][j];
                for (int c = 0; c < j; ++c) w = w - (L[i][c] * L[j][c]) * dg[c];
                L[i][j] = w / s;
            }
        }
        if (ok) {
            for (int i = 0; i < 6; ++i) {                                                // L y = -b
                double s = -total[21 + i];
                for (int c = 0; c < i; ++c) s = s - L[i][c] * x[c];
                x[i] = s;
            }
            for (int i = 0; i < 6; ++i) x[i] = x[i] / dg[i];
            for (int i = 4; i >= 0; --i) {                                               // L^T xi = z
                double s = x[i];
                for (int c = i + 1; c < 6; ++c) s = s - L[c][i] * x[c];
                x[i] = s;
            }
            for (int i = 0; i < 6; ++i) ok = ok && fabsf((float)x[i]) < INFINITY;          // a NaN fails the comparison
        }
        if (!ok) { info[SDE_ALIGN_STATUS_AT] = SDE_ALIGN_SINGULAR; return; }
        const double a0 = 0.5 * x[0], a1 = 0.5 * x[1], a2 = 0.5 * x[2];
        const double aa = (a0 * a0 + a1 * a1) + a2 * a2, den = 1.0 + aa, one = 1.0 - aa;
        float T[3][4];
        T[0][0] = (float)((one + 2.0 * (a0 * a0)) / den);
        T[0][1] = (float)((2.0 * (a0 * a1) - 2.0 * a2) / den);
        T[0][2] = (float)((2.0 * (a0 * a2) + 2.0 * a1) / den);
        T[1][0] = (float)((2.0 * (a0 * a1) + 2.0 * a2) / den);
        T[1][1] = (float)((one + 2.0 * (a1 * a1)) / den);
        T[1][2] = (float)((2.0 * (a1 * a2) - 2.0 * a0) / den);
        T[2][0] = (float)((2.0 * (a0 * a2) - 2.0 * a1) / den);
        T[2][1] = (float)((2.0 * (a1 * a2) + 2.0 * a0) / den);
        T[2][2] = (float)((one + 2.0 * (a2 * a2)) / den);
        for (int r = 0; r < 3; ++r) T[r][3] = (float)x[3 + r];
        for (int r = 0; r < 3; ++r)                                                      // sde_pose_compose's order
            for (int c = 0; c < 4; ++c) {
                float v = T[r][0] * state[c] + T[r][1] * state[4 + c] + T[r][2] * state[8 + c];
                if (c == 3) v = v + T[r][3];
                Dn[4 * r + c] = v;
            }
    }
    if ((mode & SDE_ALIGN_SCALE) && count_s >= min_count) {
        const float mean = (float)(total[29] / (double)count_s);
        state[SDE_ALIGN_SCALE_AT] = state[SDE_ALIGN_SCALE_AT] * mean;
    }
    if (mode & SDE_ALIGN_POSE) {
        float* Di = state + 16;
        for (int i = 0; i < 12; ++i) state[i] = Dn[i];
        for (int r = 0; r < 3; ++r) {                                                    // [R^T | -R^T t], term by term
            for (int c = 0; c < 3; ++c) Di[4 * r + c] = Dn[4 * c + r];
            Di[4 * r + 3] = -(Dn[r] * Dn[3] + Dn[4 + r] * Dn[7] + Dn[8 + r] * Dn[11]);
        }
    }
    info[SDE_ALIGN_STATUS_AT] = SDE_ALIGN_OK;
}

bool picture_ok(int H, int W) { return H >= 1 && W >= 1 && H <= MAX_PICTURE && W <= MAX_PICTURE; }

}  // namespace

extern "C" {

size_t sde_frame_align_ws_bytes(int H, int W) {
    if (!picture_ok(H, W)) return 0;
    return (size_t)((W + TW - 1) / TW) * (size_t)((H + TH - 1) / TH) * NV * sizeof(float);
}

int sde_frame_align_reset(float* state, sde_stream_t stream) {
    SDE_CHECK_ARG(state && ((uintptr_t)state & 3) == 0, "sde_frame_align_reset: state must be a 4-byte aligned pointer");
    hipLaunchKernelGGL(align_reset, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
    SDE_CHECK_LAUNCH("sde_frame_align_reset");
    return SDE_OK;
}

int sde_frame_align(const float* pred, int ph, int pw, const int* ymap, const int* xmap, int H, int W, const float* K, const float* model_depth,
                    const float* model_normal, float min_depth, float max_depth, float dist_tol, float scale_tol, int min_count, float damping,
                    int mode, float* state, void* workspace, size_t workspace_bytes, sde_stream_t stream) {
    SDE_CHECK_ARG(picture_ok(H, W), "sde_frame_align: H and W must lie in [1, %d] (%d x %d)", MAX_PICTURE, H, W);
    SDE_CHECK_ARG(ph > 0 && pw > 0 && (long)ph * pw <= 0x7fffffffL, "sde_frame_align: bad prediction shape (%d x %d)", ph, pw);
    SDE_CHECK_ARG(pred && ymap && xmap && K && model_depth && model_normal && state, "sde_frame_align: null pointer");
    SDE_CHECK_ARG(((uintptr_t)state & 3) == 0, "sde_frame_align: state must be 4-byte aligned");
    SDE_CHECK_ARG(mode >= 1 && mode <= 3, "sde_frame_align: mode must be SDE_ALIGN_POSE, SDE_ALIGN_SCALE or both (%d)", mode);
    SDE_CHECK_ARG(dist_tol > 0.f && scale_tol > 0.f, "sde_frame_align: dist_tol and scale_tol must be positive (%g, %g)", (double)dist_tol,
                  (double)scale_tol);                                                                    // a NaN fails the comparison
    SDE_CHECK_ARG(damping >= 0.f, "sde_frame_align: damping must not be negative (%g)", (double)damping);
    SDE_CHECK_ARG(min_count >= 6, "sde_frame_align: min_count must be at least 6 (%d)", min_count);
    SDE_CHECK_ARG(min_depth < max_depth, "sde_frame_align: min_depth must lie below max_depth (%g, %g)", (double)min_depth, (double)max_depth);
    const size_t need = sde_frame_align_ws_bytes(H, W);
    SDE_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
                  "sde_frame_align: workspace of %zu bytes, sde_frame_align_ws_bytes asks for %zu (4-byte aligned)", workspace ? workspace_bytes : (size_t)0,
                  need);
    const dim3 grid((unsigned)((W + TW - 1) / TW), (unsigned)((H + TH - 1) / TH));
    AccumP p{pred, ymap, xmap, K, model_depth, model_normal, state, (float*)workspace, H, W, ph, pw, min_depth, max_depth, dist_tol, scale_tol};
    hipLaunchKernelGGL(align_accumulate, grid, dim3(TW * TH), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(align_finish, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, (const float*)workspace, (int)(grid.x * grid.y), min_count, damping,
                       mode, state);
    SDE_CHECK_LAUNCH("sde_frame_align");
    return SDE_OK;
}

}  // extern "C"
