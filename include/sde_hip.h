/* sde_hip.h -- C ABI of libsde_hip.so: the MI355X (gfx950) kernels under the depth-training hot path.
 *
 * The reference (zzzxxxttt/SimpleDepthEstimation) is pure Python on torch; it has no FFI.  This header is
 * the NEW boundary that sits UNDER the reference's Python plugin surface (build_model / registries /
 * model(batch)->dict): every entry point replaces the stock torch call(s) named in its
 * comment (file:line in the reference).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers + sizes, no torch types.  All buffers (outputs, workspaces, partial-sum
 *     slabs) are caller-owned; nothing here allocates, frees or synchronises, so every call is legal
 *     inside a hipGraph capture.  Work is enqueued on `stream` (a hipStream_t; NULL = default stream).
 *   - return value: 0 = SDE_OK, negative = error (sde_last_error() gives the message). Never throws.
 *   - images are planar NCHW fp32 exactly as the reference's batch dict holds them; network activations
 *     are NHWC (channels-last) in fp32, bf16 or fp16, selected by the `dtype` argument (SDE_F32 / SDE_BF16 / SDE_F16).
 *   - thread safety: stateless and re-entrant given distinct streams/buffers.
 */
#ifndef SDE_HIP_H
#define SDE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sde_stream_t; /* hipStream_t */

#define SDE_MAX_CTX 4
#define SDE_F32 0
#define SDE_BF16 1
#define SDE_F16 2 /* IEEE half storage, fp32 accumulate: BASELINE.json configs[4] (needs loss scaling: sde_adam_step's scale_state) */

/* Partial-sum slabs (BatchNorm statistics, BN/bias backward reductions) must be allocated with SDE_REDUCE_ROWS extra rows:
 * slabs taller than that are first folded into their own tail by a deterministic two-level reduction. */
#define SDE_REDUCE_ROWS 32

#define SDE_RESIZE_BILINEAR_AC 0 /* F.interpolate(mode='bilinear', align_corners=True) */
#define SDE_RESIZE_NEAREST 1     /* F.interpolate(mode='nearest') */

const char* sde_last_error(void); /* message of the last failing call on this thread */
int sde_version(void);            /* ABI version, bumped on incompatible change */

/* Diagnostics: store the device's constant-rate wall clock (ticks of sde_wall_clock_khz()) into *slot, in stream order.  Captured into the step's
 * hipGraph at chosen points, the markers give the replayed step's real timeline (bench.py --marks).  Not part of the reference's surface. */
int sde_mark_time(uint64_t* slot, sde_stream_t stream);
int sde_wall_clock_khz(void); /* < 0: query failed */
/* Stream-ordered flag for the host: *dst = value (dst: host-pinned, device-visible memory; system-scope release store by one thread).  The device
 * prefetcher's hand-over between its copy stream and the training stream (no event record / wait pairs). */
int sde_store_u64(uint64_t* dst, uint64_t value, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Geometry / photometric path (fp32)
 * ------------------------------------------------------------------------------------------------- */

/* detectron2/geometry/camera.py:L40-46 resize_img.  src [planes,H,W] -> dst [planes,h,w]. */
int sde_resize(const float* src, float* dst, int planes, int H, int W, int h, int w, int mode, sde_stream_t stream);

/* detectron2/geometry/pose_utils.py:L98-137 pose_vec2mat (+ its VJP).  vec [n,6] = (tx,ty,tz,rx,ry,rz) -> mat [n,4,4]. */
int sde_pose_vec2mat(const float* vec, float* mat, int n, sde_stream_t stream);
int sde_pose_vec2mat_bwd(const float* vec, const float* dmat, float* dvec, int n, sde_stream_t stream);

/* detectron2/geometry/camera.py:L166-202 view_synthesis (= scale_intrinsics L14 + inv_intrinsics L25 + img_to_points L125 +
 * points_to_img L141 + F.grid_sample L196), with a per-sample constant translation (pose[:, :3, 3]).
 * img [B,C,H,W], depth [B,1,H,W], K [B,3,3] UNscaled intrinsics (sx,sy are the scale_intrinsics factors), pose [B,4,4].
 * Outputs (any of Z/grid/valid/fx/fy may be NULL): sampled [B,C,H,W], Z [B,1,H,W] (clamped 1e-5), grid [B,H,W,2] normalised,
 * valid [B,1,H,W] u8, fx/fy [B,H,W] int32 = floor of the un-normalised sample coordinate (bit-exact with the reference). */
int sde_view_synthesis(const float* img, const float* depth, const float* K, const float* pose, float sx, float sy, int B, int C, int H,
                       int W, float* sampled, float* Z, float* grid, uint8_t* valid, int32_t* fx, int32_t* fy, sde_stream_t stream);

/* One scale of the MonoDepth2 photometric loss, detectron2/modeling/meta_arch/MonoDepth2.py:L78-101,L116-124,L130-151
 * (rgb_consistency_loss for every context, warped + identity/auto-mask, SSIM ssim_loss.py:L34-53, min or mean reduce). */
typedef struct sde_photo_desc {
    const float* A;                /* target frame at this scale   [B,3,h,w] */
    const float* ctx[SDE_MAX_CTX]; /* context frames at this scale [B,3,h,w] */
    const float* pose[SDE_MAX_CTX];/* target->context poses        [B,4,4]   */
    const float* depth;            /* predicted depth              [B,1,h,w] */
    const float* K;                /* full-resolution intrinsics   [B,3,3]   */
    int32_t B, h, w, nctx;
    int32_t automask;              /* LOSS.AUTOMASK: add the un-warped (identity) map of every context */
    int32_t reduce_mean;           /* LOSS.PHOTOMETRIC_REDUCE: 0 = 'min', 1 = 'mean' */
    float sx, sy;                  /* scale_intrinsics factors w/W, h/H */
    float ssim_w, C1, C2;          /* LOSS.SSIM_WEIGHT, LOSS.C1, LOSS.C2 */
    const float* clip_thr;         /* LOSS.CLIP > 0: device [nmaps] thresholds mean + clip*std of each UNCLIPPED map (MonoDepth2.py:L147-149:
                                      one forward with maps != NULL and clip_thr == NULL yields them); NULL = no clipping */
} sde_photo_desc;

/* number of workgroups (= length of `partial`, and of pose_partial / (nctx*12) for backward) */
int sde_photo_num_blocks(int B, int h, int w, int backward);

/* Forward.  sampled[j] [B,3,h,w] (saved for backward), sel [B,h,w] u8 arg-min map index (order: warp0, id0, warp1, id1 ...),
 * maps (optional, may be NULL) [B,nmaps,h,w] the individual photometric maps, partial [sde_photo_num_blocks(...,0)] workspace.
 * loss_out[0] (+)= loss_scale * mean_over_pixels(reduced map).  This and sde_photo_bwd are the n = 1 case of the launch behind sde_photo_multi_fwd/_bwd. */
int sde_photo_fwd(const sde_photo_desc* d, float* const* sampled, uint8_t* sel, float* maps, float* partial, float* loss_out,
                  float loss_scale, int accumulate, sde_stream_t stream);

/* Backward w.r.t. depth and poses.  gout: device scalar (upstream gradient), multiplied by gscale.
 * d_depth [B,1,h,w]; pose_partial [sde_photo_num_blocks(...,1) * nctx * 12] workspace; d_pose[j] [B,4,4].
 * sel may be NULL only with the 'mean' reduce and no clip thresholds (nothing is read from it then); h, w >= 4 as in the forward. */
int sde_photo_bwd(const sde_photo_desc* d, const float* const* sampled, const uint8_t* sel, const float* gout, float gscale, float* d_depth,
                  int accumulate_depth, float* pose_partial, float* const* d_pose, int accumulate_pose, sde_stream_t stream);
/* Every scale of the loss (MonoDepth2.py:L78-112 loops over the four decoder scales) in ONE launch per phase: d [n] descriptors (n <= 4, same batch and
 * contexts, no clip thresholds), fine scale first; sampled [n][SDE_MAX_CTX], sel [n], partial [n] (sizes as for the single-scale calls);
 * loss_out [n] = mean over pixels of each scale's reduced map -- bit-identical to n calls of sde_photo_fwd.  Backward: gout [n] device scalars (the
 * upstream gradient of each scale's loss), d_depth [n], pose_partial [n]; d_pose [SDE_MAX_CTX] receives the SUM over the scales (written, not
 * accumulated).  The coarse scales (1/4 ... 1/64 of the pixels) are launch-sized on their own; behind the fine scale's workgroups they fill its tail. */
int sde_photo_multi_fwd(const sde_photo_desc* d, int n, float* const* sampled, uint8_t* const* sel, float* const* partial, float* loss_out,
                        sde_stream_t stream);
int sde_photo_multi_bwd(const sde_photo_desc* d, int n, const float* const* sampled, const uint8_t* const* sel, const float* gout, float* const* d_depth,
                        float* const* pose_partial, float* const* d_pose, sde_stream_t stream);
/* d_pose == NULL in sde_photo_multi_bwd leaves the per-workgroup pose partials unsummed; this call sums them (same order, same result).  Two calls so
 * that the caller can enqueue the pose side on the stream PoseNet's backward runs on (it is the only consumer), behind an event of its own. */
int sde_photo_multi_pose_finalize(const sde_photo_desc* d, int n, const float* const* pose_partial, float* const* d_pose, sde_stream_t stream);

/* The photometric AND the edge-aware smoothness term of every scale of MonoDepth2's loss loop (detectron2/modeling/meta_arch/MonoDepth2.py:L78-126,
 * modeling/losses/smoothness_loss.py:L42-80) behind one call per pass.  d [n] as for sde_photo_multi_fwd (d[s].A doubles as the smoothness term's image,
 * d[s].depth as its depth).  photo_w / smooth_w: host arrays [n] of the weights the reference multiplies each scale's term with (smooth_w NULL: no
 * smoothness term, its buffers may be NULL).  Buffers per scale: sampled / sel / photo_partial as for sde_photo_multi_fwd; sm_mean_part [B*32], sm_dn [B*h*w],
 * sm_loss_part / sm_s_part [sde_smooth_num_blocks].  per_scale [2n] receives every scale's photometric mean, then every scale's smoothness value
 * (bit-identical to sde_photo_fwd / sde_smooth_fwd); totals [2] = the two weighted sums, accumulated in scale order.  ticket: one device int, zero on
 * entry, left zero.  Backward: g_rec / g_smooth = device scalars, the upstream gradients of totals[0] / totals[1] (g_smooth NULL: photometric part only);
 * d_depth [n] is written (photometric) and then accumulated (smoothness); pose side as in sde_photo_multi_bwd. */
int sde_mono_loss_fwd(const sde_photo_desc* d, int n, const float* photo_w, const float* smooth_w, float* const* sampled, uint8_t* const* sel,
                      float* const* photo_partial, float* const* sm_mean_part, float* const* sm_dn, float* const* sm_loss_part, float* const* sm_s_part,
                      float* per_scale, float* totals, int* ticket, sde_stream_t stream);
int sde_mono_loss_bwd(const sde_photo_desc* d, int n, const float* photo_w, const float* smooth_w, const float* const* sampled, const uint8_t* const* sel,
                      const float* g_rec, const float* g_smooth, const float* const* sm_mean_part, const float* const* sm_dn, const float* const* sm_s_part,
                      float* const* d_depth, float* const* pose_partial, float* const* d_pose, sde_stream_t stream);
/* The smoothness half of sde_mono_loss_bwd on its own (a caller that forks the pose side to another stream between the two halves): d_depth[s] (+)= ... */
int sde_smooth_multi_bwd(const sde_photo_desc* d, int n, const float* smooth_w, const float* g_smooth, const float* const* sm_mean_part, const float* const* sm_dn,
                         const float* const* sm_s_part, float* const* d_depth, int accumulate, sde_stream_t stream);

/* Stand-alone SSIM distance map, the callable module of detectron2/modeling/losses/ssim_loss.py:L6-53:
 * out[b,c,h,w] = clamp((1 - SSIM(x, y)) / 2, 0, 1) with ReflectionPad2d(1) + 3x3 mean; x, y, out planar [B,C,H,W] fp32 (the training path
 * evaluates SSIM inside sde_photo_fwd / sde_photo_bwd).  Backward: dx and/or dy (either may be NULL) for the upstream gradient gout [B,C,H,W];
 * coef_ws: [B*C*H*W][4] floats of workspace, 16-byte aligned. */
int sde_ssim_fwd(const float* x, const float* y, int B, int C, int H, int W, float C1, float C2, float* out, sde_stream_t stream);
int sde_ssim_bwd(const float* x, const float* y, const float* gout, int B, int C, int H, int W, float C1, float C2, float* coef_ws, float* dx, float* dy,
                 sde_stream_t stream);

/* detectron2/modeling/losses/smoothness_loss.py:L42-80.  depth [B,1,h,w], img [B,3,h,w].
 * mean_part [B*32], dn [B,h,w], loss_part/s_part [sde_smooth_num_blocks] are caller workspaces that backward re-reads.
 * loss_out[0] (+)= loss_scale * smoothness_loss.  These two entries are the n = 1 case of the smoothness launches behind sde_mono_loss_fwd/_bwd. */
int sde_smooth_num_blocks(int B, int h, int w);
int sde_smooth_fwd(const float* depth, const float* img, int B, int h, int w, float* mean_part, float* dn, float* loss_part, float* s_part,
                   float* loss_out, float loss_scale, int accumulate, sde_stream_t stream);
int sde_smooth_bwd(const float* depth, const float* dn, const float* mean_part, const float* s_part, const float* gout, float gscale, int B,
                   int h, int w, float* d_depth, int accumulate, sde_stream_t stream);

/* detectron2/modeling/losses/losses.py:L5-13 silog_loss against resize_img(depth_gt, 'nearest') (Supervised.py:L44-45), fused:
 * est [B,1,h,w], gt [B,1,H,W] full resolution (nearest-sampled in-kernel), mask gt > 1; H >= h, W >= w (both entries check it).  No compaction, no host sync.
 * part [sde_silog_num_blocks*3] workspace; stats[4] = (count, E[d], E[d^2], loss).  These two entries are the n = 1, weight 1 case of the launches behind
 * sde_silog_multi_fwd/_bwd. */
int sde_silog_num_blocks(int B, int h, int w);
int sde_silog_fwd(const float* est, const float* gt, int B, int h, int w, int H, int W, float variance_focus, float* part, float* stats,
                  sde_stream_t stream);
int sde_silog_bwd(const float* est, const float* gt, const float* stats, const float* gout, float gscale, float variance_focus, int B, int h,
                  int w, int H, int W, float* d_est, int accumulate, sde_stream_t stream);
/* The same loss summed over up to SDE_SILOG_MAX_SCALES prediction scales against ONE ground truth (Supervised.py:L42-47: the four decoder scales,
 * weight 1/4 each) in one launch per phase: total[0] = sum_k weight[k] * SILog(est[k], nearest(gt)), stats [n][4] as above per scale (bit-identical to
 * the single-scale call), part: [sde_silog_multi_num_blocks][3].  Backward writes d_est[k] = gout * gscale * weight[k] * dSILog_k/d est[k]. */
#define SDE_SILOG_MAX_SCALES 4
int sde_silog_multi_num_blocks(int B, const int* h, const int* w, int n);
int sde_silog_multi_fwd(const float* const* est, const float* gt, int B, const int* h, const int* w, const float* weight, int n, int H, int W,
                        float variance_focus, float* part, float* stats, float* total, sde_stream_t stream);
int sde_silog_multi_bwd(const float* const* est, const float* gt, const float* stats, const float* gout, float gscale, float variance_focus, int B,
                        const int* h, const int* w, const float* weight, int n, int H, int W, float* const* d_est, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Convolution engine (NHWC activations, fp32 or bf16 storage, fp32 accumulate)
 * ------------------------------------------------------------------------------------------------- */
#define SDE_SRC_PLAIN 0   /* input tensor as stored */
#define SDE_SRC_UPCAT 1   /* cat(F.interpolate(x0, scale 2, nearest), x1) -- depth_decoder.py:L102-105 -- never materialised */
#define SDE_SRC_ZEROINS 2 /* x0 with zeros inserted between pixels: data-gradient of a stride-2 convolution */
#define SDE_ACT_NONE 0
#define SDE_ACT_ELU 1
#define SDE_ACT_RELU 2

/* Input side of a convolution.  The virtual input is [Bn, IH, IW, C0+C1]; channel counts are multiples of 16 bytes. */
typedef struct sde_conv_desc {
    const void* x0; /* [Bn, H0, W0, C0] */
    const void* x1; /* [Bn, IH, IW, C1] (SDE_SRC_UPCAT only) or NULL */
    int32_t dtype;  /* SDE_F32 / SDE_BF16 (storage type of x0, x1, weights and outputs) */
    int32_t C0, C1, H0, W0, IH, IW, src_mode;
    int32_t KH, KW, stride, pad;
    int32_t reflect; /* 1: ReflectionPad2d(pad) (depth_decoder.py:L40-43), 0: zero padding */
    int32_t Bn, OH, OW;
} sde_conv_desc;

/* master fp32 OIHW weight [Cout,Cin,KH,KW] -> K-major operand in `dtype`:
 *   for_dgrad = 0: [Cout_pad][KH][KW][Cin_pad]            (forward and weight-gradient layout)
 *   for_dgrad = 1: [Cin_pad][KH][KW][Cout_pad], taps flipped (data-gradient operand) */
int sde_pack_weight(const float* w, void* out, int dtype, int Cout, int Cin, int KH, int KW, int Cin_pad, int Cout_pad, int for_dgrad,
                    sde_stream_t stream);

/* Both operands of every layer of a model in ONE launch (the weights change once per optimizer step).  items: DEVICE array of n layers,
 * built once; a workgroup transposes one (32 output channels x sde-chosen input-channel block x all taps) tile through LDS;
 * `end` = exclusive prefix sum of sde_pack_item_blocks() over the layers, total_blocks = items[n-1].end. */
typedef struct sde_pack_item {
    const float* src; /* master fp32 weights (SDE_W_TWIN16: their 16-bit twin): [Cout][Cin][KH][KW] (src_layout SDE_W_OIHW) or [Cout][KH][KW][Cin] (SDE_W_OHWI, channels-last) */
    void* dst_fwd;    /* [Cout_pad][KH][KW][Cin_pad] in `dtype` (or NULL) */
    void* dst_dgrad;  /* [Cin_pad][KH][KW][Cout_pad], taps flipped (or NULL) */
    int32_t Cout, Cin, KH, KW, Cin_pad, Cout_pad;
    int32_t src_layout, reserved;
    int64_t end;
} sde_pack_item;
#define SDE_W_OIHW 0 /* torch's default memory order of a conv weight */
#define SDE_W_OHWI 1 /* torch.channels_last order of the same [Cout,Cin,KH,KW] tensor: K-major like the packed operands and the gradient slabs */
#define SDE_W_TWIN16 2 /* src is NOT fp32 but the 16-bit twin of a channels-last master slot (sde_adam_step_twin), i.e. the forward operand itself: only dst_dgrad is
                        * written (dst_fwd is ignored).  Needs a 16-bit `dtype`, Cin_pad == Cin, Cout_pad == Cout, both multiples of 8, src and dst_dgrad 16-byte aligned. */
int sde_pack_item_blocks(int Cout_pad, int Cin_pad, int KH, int KW);
int sde_pack_weights_batched(const sde_pack_item* items_dev, int n, long total_blocks, int dtype, sde_stream_t stream);

/* y[Bn,OH,OW,ldy] = act(conv(virtual input, w_packed) + bias); channels >= Cout of y are written as zeros.
 * Replaces nn.Conv2d (+ReflectionPad2d, +upsample/cat, +nn.ELU) forward -- resnet_encoder.py:L91-97, depth_decoder.py:L21-53,
 * PoseNet.py:L13-16 -- and, with the flipped operand of sde_pack_weight(for_dgrad=1), their data-gradient.
 * stats (optional): [sde_conv_fwd_tiles_m + SDE_REDUCE_ROWS][Cout][2] per-tile (sum, sum of squares) of the stored outputs, for BatchNorm. */
int sde_conv_fwd(const sde_conv_desc* d, const void* w_packed, const float* bias, int act, void* y, int Cout, int ldy, float* stats,
                 sde_stream_t stream);
/* The same with a caller-owned fp32 workspace of sde_conv_fwd_ws_bytes() bytes (0: not needed): small-M, long-K layers then run split-K
 * (K cut into up to 8 ranges, partial tiles summed in a fixed order by a finishing kernel that also applies bias / activation / statistics). */
size_t sde_conv_fwd_ws_bytes(const sde_conv_desc* d, int ldy);
int sde_conv_fwd_ws(const sde_conv_desc* d, const void* w_packed, const float* bias, int act, void* y, int Cout, int ldy, float* stats, void* ws,
                    size_t ws_bytes, sde_stream_t stream);
/* Data gradient of a stride-1 convolution whose INPUT was relu(BatchNorm(y_bn)) with no residual and no other consumer (torchvision Bottleneck:
 * conv2 <- bn1, conv3 <- bn2; BasicBlock: conv2 <- bn1 -- detectron2/layers/resnet_encoder.py:L88-99 wraps those blocks): the GEMM is the one
 * sde_conv_fwd runs for the same descriptor (d = the dgrad view: source dz, flipped operand), and its epilogue takes over the first pass of
 * BatchNorm's backward: gm [M][ldy] = (fma(y_bn, scale, shift) > 0) * g is stored instead of g, and part [rows][Cout][2] receives the
 * per-workgroup sums (sum gm, sum gm * xhat), xhat = (y_bn - mean) * rstd; bnp [4][Cout] = (mean, rstd, scale, shift) as sde_bn_finalize wrote it.
 * sde_conv_dgrad_bnbwd_rows: rows of that slab, or 0 when the dispatcher has no fused form for this layer (fp32, split-K, stride 2, channel
 * counts that are not multiples of 64, narrow layers): the caller then runs sde_conv_fwd and sde_bn_bwd.  Follow with sde_bn_bwd_from_part. */
int sde_conv_dgrad_bnbwd_rows(const sde_conv_desc* d, int Cout, int ldy);
int sde_conv_dgrad_bnbwd(const sde_conv_desc* d, const void* w_packed, void* gm, int Cout, int ldy, const void* bn_y, const float* bnp, float* part,
                         sde_stream_t stream);
/* The residual form (torchvision Bottleneck, resnet_encoder.py:L88-99: out = relu(bn3(y_bn) + identity) feeds conv1 of the next block AND that block's
 * skip path): the data gradient of that conv1 takes over the WHOLE reduce pass of bn3's backward -- gm = (g + res_grad) * (bn_out > 0), res_grad the
 * gradient arriving over the skip path, bn_out the block output (the mask), and the same partial slab.  Persistent GEMM and LDS-halo 3x3 kernel
 * (BasicBlock: bn2 -> conv1 of the next block); rows = 0 where neither runs the layer. */
int sde_conv_dgrad_bnbwd_res_rows(const sde_conv_desc* d, int Cout, int ldy);
int sde_conv_dgrad_bnbwd_res(const sde_conv_desc* d, const void* w_packed, void* gm, int Cout, int ldy, const void* bn_y, const float* bnp, float* part,
                             const void* res_grad, const void* bn_out, sde_stream_t stream);
/* The dispatcher's queries -- sde_conv_fwd_tiles_m (rows of the statistics slab), sde_conv_fwd_variant (the kernel: <BM><BN> register-staged tiles,
 * 3128<BN> LDS-halo 3x3, 5<Cin><ldy> narrow-input halo, 7<BM><BN> persistent GEMM), sde_conv_fwd_ws_bytes, sde_conv_dgrad_bnbwd_rows / _res_rows,
 * sde_conv_wgrad_variant and sde_conv_wgrad_splits -- read the one route the launch itself takes (csrc/conv.hip: route_fwd, route_wgrad).
 * All of them answer 0 for a NULL descriptor or one the launch would refuse, with the reason in sde_last_error(); the launch then refuses the
 * same descriptor with SDE_ERR_ARG, so a caller that sizes its buffers by a 0 never reaches a kernel. */
int sde_conv_fwd_tiles_m(const sde_conv_desc* d, int ldy);
int sde_conv_fwd_variant(const sde_conv_desc* d, int ldy);
/* Tuning / test knob: the LDS-halo 3x3 kernel is used when a launch has at least this many workgroups (default 192; 0 = whenever it
 * applies, negative = never).  Returns the previous value.  Results do not depend on it beyond fp32 summation order. */
int sde_conv_set_halo_min_blocks(int min_blocks);
/* Dispatcher options (process-wide; A/B measurements and tests): returns the previous value, negative on a bad key / value.  Results do
 * not depend on them beyond fp32 summation order.
 *   SDE_OPT_PGEMM        1 (default): layers with 64-channel-multiple inputs run on the persistent LDS-DMA GEMM (csrc/pgemm.hip); 0: never
 *   SDE_OPT_PGEMM_DEPTH  stages of its LDS ring: 3 (default) or 4
 *   SDE_OPT_PGEMM_3X3    1: it also takes the 3x3 stride-1 layers the LDS-halo kernel would get (default 0) */
#define SDE_OPT_PGEMM 1
#define SDE_OPT_PGEMM_DEPTH 2
#define SDE_OPT_PGEMM_3X3 3
#define SDE_OPT_PGEMM_TILE 4   /* force its tile: 64064, 128064, 128128; 0 (default) = chosen per layer */
#define SDE_OPT_SPLITK 5       /* 1 (default): small-M, long-K layers cut K into up to 8 ranges (sde_conv_fwd_ws); 0: never */
#define SDE_OPT_WGRAD_BLOCKS 6 /* workgroup target of the weight-gradient GEMM's pixel splits (default 256 = one per CU) */
#define SDE_OPT_WGRAD_HALO 7   /* 1 (default): the 3x3 stride-1 layers with <= 96 input and <= 32 output channels take the LDS-halo weight-gradient
                                  kernel (csrc/wgrad_halo.hip); 0: the generic kernel */
#define SDE_OPT_CONV_SMALL 8   /* 1 (default): 3x3 stride-1 layers with 8 / 16 / 32 input channels and >= 16 K output pixels take the narrow-input halo
                                  kernel (csrc/conv_halo_small.hip) in the forward and data-gradient passes; 0: the generic kernel */
#define SDE_OPT_WGRAD_DMA 9    /* 1 (default): layers with 64-channel-multiple inputs and outputs (zero padding, no concat) take the LDS-DMA weight-gradient
                                  kernel (csrc/wgrad_dma.hip); 0: the register-staged kernel */
#define SDE_OPT_BNBWD_FUSE 10  /* 1 (default): sde_conv_dgrad_bnbwd_rows reports the layers whose data gradient can carry BatchNorm's backward reduction
                                * in its epilogue; 0: it reports none (the separate bn_bwd_reduce pass runs everywhere: A/B, tests) */
#define SDE_OPT_CU_RESERVE 11  /* compute units the persistent kernels (pgemm, chalo, whalo) leave free: their grids are sized for (CUs - n) instead of every CU.
                                * 0 (default); a multiple of 8 <= 128.  For data-parallel runs: RCCL's channel kernels otherwise wait for a resident workgroup to end */
#define SDE_OPT_WGRAD_DMA_RING 12 /* LDS ring of the LDS-DMA weight-gradient kernel: 0 (default) = 64 pixels x 3 stages (72 KB per workgroup), 1 = 32 pixels x 4
                                  * stages (48 KB), 2 = 32 x 3 (36 KB).  The slim forms leave room for two workgroups of the persistent GEMM on the compute unit
                                  * beside one of these (training forks these launches next to the data-gradient chain); the slabs are bit-identical */
#define SDE_OPT_PGEMM_PER_CU 13  /* workgroups per compute unit the persistent GEMM sizes its grid for: 2, 3 or 4 (default 4 = whatever its LDS ring allows, 3 for
                                  * the 64 x 64 tile).  It also decides the rows of the BatchNorm partial slabs (sde_conv_fwd_tiles_m, sde_conv_dgrad_bnbwd_rows):
                                  * set it before asking for them.  Changes the summation order of those partial rows, no GEMM output */
int sde_conv_set_option(int key, int value);
/* Dynamic LDS bytes per workgroup of the kernels that share a compute unit during the backward pass (the data-gradient chain on one queue, the
 * weight gradients beside it), for budget checks: variant = ring depth (PGEMM, 64 x 64 tile), SDE_OPT_WGRAD_DMA_RING value (WGRAD_DMA),
 * 10 * (Cin / 16) + (Cout > 16 ? 2 : 1) (WGRAD_HALO), 0 for the others (WGRAD_STAGED: its 16-bit form; WGRAD_REDUCE: the most a launch asks for).
 * Negative on a bad kind / variant.  Host-only: touches no device. */
#define SDE_KERNEL_PGEMM 1
#define SDE_KERNEL_WGRAD_DMA 2
#define SDE_KERNEL_WGRAD_HALO 3
#define SDE_KERNEL_WGRAD_STAGED 4
#define SDE_KERNEL_WGRAD_SUM 5
#define SDE_KERNEL_WGRAD_REDUCE 6
int sde_kernel_lds_bytes(int kind, int variant);

/* dW (master fp32 OIHW, [Cout,Cin_real,KH,KW]) (+)= sum over output pixels of dy^T * im2col(virtual input).
 * slab: caller workspace [splits][Cout][KH*KW*(C0+C1)] fp32, splits = sde_conv_wgrad_splits(d, Cout): one fp32 partial per pixel range,
 * summed in a fixed order (stacks taller than SDE_WGRAD_FOLD_ROWS as that many chunk sums first) -- bit-reproducible, no atomics. */
#define SDE_WGRAD_FOLD_ROWS 16
int sde_conv_wgrad_splits(const sde_conv_desc* d, int Cout);
/* Which weight-gradient GEMM sde_conv_wgrad / sde_conv_wgrad_partial take for this layer (the dispatcher's own predicates; tests pin their
 * cases with it): 1 = halo kernel (wgrad_halo.hip), 2 = LDS-DMA kernel (wgrad_dma.hip), 3 = register-staged kernel (conv.hip); 0 = bad descriptor. */
#define SDE_WGRAD_HALO_KERNEL 1
#define SDE_WGRAD_DMA_KERNEL 2
#define SDE_WGRAD_STAGED_KERNEL 3
int sde_conv_wgrad_variant(const sde_conv_desc* d, int Cout, int ldd);
int sde_conv_wgrad(const sde_conv_desc* d, const void* dy, int Cout, int ldd, int Cin_real, float* slab, int splits, float* dw, int accumulate,
                   sde_stream_t stream);

/* Deferred form for training loops: sde_conv_wgrad_partial runs the GEMM only (slab: [splits][Cout][KH*KW*Cin], no scratch rows);
 * sde_wgrad_reduce_batched then sums the slabs of MANY layers in one launch per <= 120 items, in the same order as sde_conv_wgrad
 * (results are bit-identical).  `items` is a HOST array: it is copied into the kernel arguments, so nothing has to outlive the call. */
int sde_conv_wgrad_partial(const sde_conv_desc* d, const void* dy, int Cout, int ldd, float* slab, int splits, sde_stream_t stream);
typedef struct sde_wreduce_item {
    const float* slab; /* the slab stack sde_conv_wgrad_partial filled (device) */
    float* dw;         /* master fp32 gradient of the [Cout,Cin_real,KH,KW] weight (device), in OIHW or OHWI memory order */
    int32_t rows /* = splits */, Cout, KHW, Cin_pad, Cin_real;
    int32_t accumulate; /* bit 0: add to dw instead of overwriting; bit 1 (SDE_WREDUCE_OHWI): dw is in OHWI (channels-last) order */
} sde_wreduce_item;
#define SDE_WREDUCE_ACCUMULATE 1
#define SDE_WREDUCE_OHWI 2
int sde_wgrad_reduce_batched(const sde_wreduce_item* items, int n, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Layers around the convolutions (NHWC, `dtype` storage, fp32 math)
 * ------------------------------------------------------------------------------------------------- */
/* (img - mean)/std (Supervised.py:L39, MonoDepth2.py:L60) fused with NCHW fp32 -> NHWC `dtype`, channel padding and the optional
 * torch.flip(image,[3]) of DepthResNet.py:L52-53.  mean/std may both be NULL (PoseNet input: no normalisation). */
int sde_prep_input(const float* img, const float* mean, const float* std_, int B, int C, int H, int W, int Cpad, int flip, int dtype, void* out,
                   sde_stream_t stream);

/* Training-mode nn.BatchNorm2d of torchvision's ResNet (resnet_encoder.py:L92, blocks L94-97): batch statistics from the
 * convolution's stats slab -> bnp [4][C] = (mean, rstd, scale, shift); running stats updated in place (momentum, unbiased var). */
int sde_bn_finalize(const float* part, int tiles, int C, long count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                    float momentum, float eps, float* bnp, sde_stream_t stream);
int sde_bn_eval_params(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, int C, float* bnp,
                       sde_stream_t stream);
/* out = [relu](y*scale + shift [+ residual]) */
int sde_bn_apply(const void* y, const float* bnp, const void* residual, int relu, long M, int C, int dtype, void* out, sde_stream_t stream);
/* sde_bn_finalize + sde_bn_apply in one launch (same arguments, count = M rows), for 16-bit types, C % 64 == 0 and at most 256 slab rows
 * (sde_bn_finalize_apply_ok): every workgroup reduces the slab columns of its own 64 channels, redundantly and in a fixed order. */
int sde_bn_finalize_apply_ok(int tiles, int C, int dtype);
/* sde_bn_bwd fuses its finalize and apply passes the same way; for the big layers its reduce pass runs 1024-thread workgroups so that the partial
 * slab stays within 256 rows.  sde_bn_set_fuse(0) turns the fusion off, (2) keeps it for the short slabs only (A/B, tests).  Returns the previous value. */
int sde_bn_set_fuse(int on);
int sde_bn_finalize_apply(const float* part, int tiles, int C, long count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, float* bnp, const void* y, const void* residual, int relu, int dtype, void* out, sde_stream_t stream);
/* BatchNorm(+ReLU, +residual) backward.  The normalised output may have up to three consumers whose gradients arrive separately
 * (dout, dout1, dout2; the latter two may be NULL): they are summed on the fly.  gm [M,C] (workspace, required when relu is set or more than
 * one gradient is given) receives dz = relu'(out) * (sum of the gradients) -- which is also the gradient of the residual input.
 * out: the saved forward output (ReLU mask).  With relu set and out == NULL the mask is re-derived from y and bnp as fma(y, scale, shift) > 0 --
 * valid only when the forward had NO residual (then it equals out > 0, and one activation-sized stream less is read).
 * part: [sde_reduce_num_blocks(M, C) + SDE_REDUCE_ROWS][C][2] workspace, coef: [2][C] workspace.  dy [M,C]; dgamma/dbeta [C] (+)=. */
int sde_reduce_num_blocks(long M, int C);
int sde_bn_bwd(const void* dout, const void* dout1, const void* dout2, const void* out, const void* y, const float* bnp, const float* gamma, int relu,
               long M, int C, int dtype, float* part, float* coef, float* dgamma, float* dbeta, int accumulate_params, void* gm, void* dy,
               sde_stream_t stream);
/* The same backward with the reduce pass already done by the data-gradient GEMM that produced the incoming gradient (sde_conv_dgrad_bnbwd):
 * gm [M,C] = relu'(bn(y)) * g as that GEMM stored it, part [rows + SDE_REDUCE_ROWS][C][2] = its per-workgroup (sum gm, sum gm * xhat).  Runs the
 * finalize and apply passes only (one launch for rows <= 256 and C % 64 == 0, as sde_bn_bwd).  dy [M,C]; dgamma/dbeta [C] (+)=; coef [2][C]. */
int sde_bn_bwd_from_part(const float* part, int rows, const void* gm, const void* y, const float* bnp, long M, int C, int dtype, float* coef,
                         float* dgamma, float* dbeta, int accumulate_params, void* dy, sde_stream_t stream);

/* nn.MaxPool2d(3, 2, 1) (resnet_encoder.py:L94).  idx: [B,OH,OW,C] u8 arg-max saved for backward. */
int sde_maxpool_fwd(const void* x, int B, int H, int W, int C, int dtype, void* out, uint8_t* idx, sde_stream_t stream);
int sde_maxpool_bwd(const void* dout, const uint8_t* idx, int B, int H, int W, int C, int dtype, void* dx, sde_stream_t stream);
/* ... with the gradients of two consumers of the pooled tensor summed on the fly (dout1 may be NULL) */
int sde_maxpool_bwd_sum(const void* dout, const void* dout1, const uint8_t* idx, int B, int H, int W, int C, int dtype, void* dx, sde_stream_t stream);

/* dz = dout * act'(out) (nn.ELU / nn.ReLU backward) fused with the bias gradient dbias[c] (+)= sum_rows dz[:, c], c < Cbias.
 * dz and/or dbias may be NULL; part: [sde_reduce_num_blocks(M, C) + SDE_REDUCE_ROWS][C] workspace (needed when dbias != NULL). */
int sde_act_bwd_bias(const void* dout, const void* out, int act, long M, int C, int dtype, void* dz, float* part, float* dbias, int Cbias, int accumulate,
                     sde_stream_t stream);
/* ... of an activation with two consumers (a decoder level feeds its disparity head and the next level): dz = act'(out) * (dout + dout1), dout1 may be NULL */
int sde_act_bwd_bias_sum(const void* dout, const void* dout1, const void* out, int act, long M, int C, int dtype, void* dz, float* part, float* dbias, int Cbias,
                         int accumulate, sde_stream_t stream);
/* part given but dbias == NULL: only the per-workgroup column partials are written ([sde_reduce_num_blocks(M, C)][C]); this call then sums the partial
 * slabs of MANY layers in one launch (out[c] (+)= sum_rows part[r][c], c < C, every item exactly as the per-layer finalize sums it).  The per-layer
 * finalize is a launch-sized kernel on the backward pass's serial chain that nothing downstream waits for.  `items` is a HOST array (copied by value). */
typedef struct sde_colsum_item {
    const float* part; /* [rows][ld] fp32 partial slab (device) */
    float* out;        /* [C] destination (device) */
    int32_t rows, ld, C, accumulate;
} sde_colsum_item;
int sde_colsum_finalize_batched(const sde_colsum_item* items, int n, sde_stream_t stream);

/* Backward of ReflectionPad2d(1) [+ nearest x2 upsample + channel concat] (depth_decoder.py:L40-47,L102-105):
 * dxp [B,H+2,W+2,C] (gradient w.r.t. the padded virtual input, from the data-gradient GEMM) ->
 * upcat=0: dx0 [B,H,W,C];  upcat=1: dx0 [B,H/2,W/2,C0], dx1 [B,H,W,C-C0]. */
int sde_refl_fold(const void* dxp, int B, int H, int W, int C, int C0, int upcat, int dtype, void* dx0, void* dx1, sde_stream_t stream);

/* nn.Softplus + disp_to_depth(min_depth, max_depth)[1] (+ torch.flip of the output) -- depth_decoder.py:L9-18,L108, DepthResNet.py:L57-60.
 * y [B,H,W,ld] (channel 0 is the disparity logit) -> depth [B,1,H,W] fp32; backward writes dy [B,H,W,ld] (channels > 0 zero). */
int sde_depth_head_fwd(const void* y, int B, int H, int W, int ld, float min_depth, float max_depth, int flip, int dtype, float* depth, sde_stream_t stream);
int sde_depth_head_bwd(const void* y, const float* ddepth, int B, int H, int W, int ld, float min_depth, float max_depth, int flip, int dtype, void* dy,
                       sde_stream_t stream);
/* ... also producing the bias gradient of the one-channel convolution in front of the head (depth_decoder.py:L95-97 `dispconv`): dbias[0] (+)= sum of the
 * logit gradients as stored in dy.  part: [sde_depth_head_bias_blocks(B, H, W)] floats; part and dbias are given together or both NULL. */
int sde_depth_head_bias_blocks(int B, int H, int W);
int sde_depth_head_bwd_bias(const void* y, const float* ddepth, int B, int H, int W, int ld, float min_depth, float max_depth, int flip, int dtype, void* dy,
                            float* part, float* dbias, int accumulate, sde_stream_t stream);

/* nn.GroupNorm(G) + activation: relu = 0 none, 1 nn.ReLU (PoseNet.py:L13-20), 2 nn.ELU (layers01.py:L33-40).
 * part: [B][SDE_GN_CHUNKS][C][2] workspace, gnp: [B][G][2] (mean, rstd) saved for backward, coef: [B][G][2] workspace. */
#define SDE_GN_CHUNKS 64
int sde_gn_relu_fwd(const void* x, const float* gamma, const float* beta, int B, int HW, int C, int G, float eps, int relu, int dtype, float* part, float* gnp,
                    void* out, sde_stream_t stream);
int sde_gn_relu_bwd(const void* dout, const void* out, const void* x, const float* gnp, const float* gamma, int B, int HW, int C, int G, int relu, int dtype,
                    float* part, float* coef, float* dgamma, float* dbeta, int accumulate_params, void* dx, sde_stream_t stream);
/* The same with a residual input: the normalised tensor is x + res (summed in fp32, never materialised) -- layers01.py:L74-76 ResidualConv:
 * normalize(x_out + shortcut).  res may be NULL (= the calls above); with res, C / (16-byte group) must divide 256.  Backward: dx is the
 * gradient of BOTH x and res. */
int sde_gn_relu_res_fwd(const void* x, const void* res, const float* gamma, const float* beta, int B, int HW, int C, int G, float eps, int relu, int dtype,
                        float* part, float* gnp, void* out, sde_stream_t stream);
int sde_gn_relu_res_bwd(const void* dout, const void* out, const void* x, const void* res, const float* gnp, const float* gamma, int B, int HW, int C, int G, int relu,
                        int dtype, float* part, float* coef, float* dgamma, float* dbeta, int accumulate_params, void* dx, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * BTS decoder operators (csrc/bts.hip; detectron2/modeling/depth_net/BTSNet.py:L39-275), NHWC activations in `dtype`, 16-byte channel groups
 * ------------------------------------------------------------------------------------------------- */
/* Dilated 3x3 convolution (atrous_conv, L39-64: stride 1, pad = dilation d) as space-to-batch around the conv engine:
 * split: x [B,H,W,C] -> sub [B*d*d, Hs, Ws, C], Hs = ceil(H/d), Ws = ceil(W/d), sub[(b*d+ph)*d+pw, i, j] = x[b, i*d+ph, j*d+pw] (zero beyond the map);
 * a 3x3 pad-1 convolution of sub (sde_conv_fwd, and its data and weight gradients) is then the dilated convolution of x, and
 * merge: sub [B*d*d, Hs, Ws, C] -> out [B,H,W,C] crops it back.  Each is the other's backward. */
int sde_dilate_split(const void* x, int B, int H, int W, int C, int d, int dtype, void* out, sde_stream_t stream);
int sde_dilate_merge(const void* sub, int B, int H, int W, int C, int d, int dtype, void* out, sde_stream_t stream);
/* F.interpolate(scale_factor=2, mode='nearest') of `upconv` (L67-79): x [B,H,W,C] -> out [B,2H,2W,C]; backward: dx [B,H,W,C] = 2x2 block sums of dout */
int sde_upsample2_fwd(const void* x, int B, int H, int W, int C, int dtype, void* out, sde_stream_t stream);
int sde_upsample2_bwd(const void* dout, int B, int H, int W, int C, int dtype, void* dx, sde_stream_t stream);
/* torch.cat(pieces, dim=1) of bts.forward (L208-268): P pixels, pieces in channel order; an activation piece is [P][ld] in `dtype` with C real channels,
 * an f32map piece a planar [B,1,H,W] fp32 map (C = 1, ld ignored).  out [P][Ct], Ct = the real channels rounded up to the 16-byte group, zero filled.
 * Backward: the same piece list names the destinations; activation destinations get zeros in channels [C, ld).  The list is copied by value. */
#define SDE_CAT_MAX 6
typedef struct sde_cat_piece {
    void* p;
    int32_t C, ld, f32map, reserved;
} sde_cat_piece;
int sde_cat_fwd(const sde_cat_piece* pieces, int n, long P, int Ct, int dtype, void* out, sde_stream_t stream);
int sde_cat_bwd(const void* dout, long P, int Ct, int dtype, const sde_cat_piece* grads, int n, sde_stream_t stream);
/* Batch statistics of a stored tensor x [M][C] (first_bn over a concatenation, L44-47): part [sde_channel_stats_tiles(M) + SDE_REDUCE_ROWS][C][2]
 * receives per-tile (sum, sum of squares) over SDE_STATS_ROWS rows each -- the slab sde_bn_finalize reads. */
#define SDE_STATS_ROWS 256
int sde_channel_stats_tiles(long M);
int sde_channel_stats(const void* x, long M, int C, int dtype, float* part, sde_stream_t stream);
/* nn.ReLU (L53): y = max(x, 0) over n elements (backward: sde_act_bwd_bias with SDE_ACT_RELU) */
int sde_relu_fwd(const void* x, long n, int dtype, void* y, sde_stream_t stream);
/* reduction_1x1's plane head (L110-122) + F.normalize + local_planar_guidance (L126-148) + / max_depth (+ nearest down-sampling by ds), fused:
 * y [B,h,w,ld] = the plane_params convolution's output (channels 0..2 the logits) -> full [B,1,h*r,w*r] fp32, and with ds > 0
 * down [B,1,h*r/ds,w*r/ds] = full[:, :, ds*i, ds*j] (F.interpolate(scale_factor=1/ds, mode='nearest')).  No clamp on the plane denominator.
 * Backward: dfull and / or ddown (either may be NULL; the two consumers' gradients add) -> dy [B,h,w,ld] (channels >= 3 zero). */
int sde_lpg_fwd(const void* y, int B, int h, int w, int ld, int r, float max_depth, int ds, int dtype, float* full, float* down, sde_stream_t stream);
int sde_lpg_bwd(const void* y, const float* dfull, const float* ddown, int B, int h, int w, int ld, int r, float max_depth, int ds, int dtype, void* dy,
                sde_stream_t stream);
/* Sigmoid depth heads (reduc1x1 `final`, L88-95; get_depth, L195-196,L272-274): out [B,1,H,W] fp32 = sigmoid(y[...,0]) * scale, then
 * (* focal[b]) / focal_div when focal (device [B]) is given; flip mirrors the output along x.  Backward writes dy [B,H,W,ld] (channels > 0 zero). */
int sde_sigmoid_head_fwd(const void* y, int B, int H, int W, int ld, float scale, const float* focal, float focal_div, int flip, int dtype, float* out,
                         sde_stream_t stream);
int sde_sigmoid_head_bwd(const void* y, const float* dout, int B, int H, int W, int ld, float scale, const float* focal, float focal_div, int flip, int dtype,
                         void* dy, sde_stream_t stream);


/* ---------------------------------------------------------------------------------------------------
 * GoogleResNet operators (csrc/google.hip; detectron2/modeling/depth_net/GoogleResNet.py, detectron2/layers/layer_norm.py), NHWC activations
 * in fp32 or bf16 (SDE_F16 is refused), 16-byte channel groups.  No atomics: repeated runs give identical bits.
 * ------------------------------------------------------------------------------------------------- */
/* RandLayerNorm (layer_norm.py:L7-33) of y [B,HW,C] (C <= 2048 channels, the first Cr real): per-(sample, channel) mean and unbiased variance
 * over HW >= 2 pixels; in training (train = 1) both are multiplied by 1 + fmod(z * s, 2s) with z [2][B][Cr] (mean draws, then variance draws) and
 * s = *stddev read from device memory (s == 0: factor 1 exactly); out = gamma * (y - mean) * rsqrt(var + eps) + beta [+ res] [-> ReLU], pad
 * channels zero.  part: [B][SDE_RLN_CHUNKS][C][2] workspace; rlnp [B][C][2] = (mean, rstd) as used, saved for backward.  Two launches.
 * sde_randln_chunks(HW): pixel chunks per sample (workgroups per sample of every launch). */
#define SDE_RLN_CHUNKS 32
int sde_randln_chunks(int HW);
int sde_randln_fwd(const void* y, const void* res, const float* gamma, const float* beta, const float* z, const float* stddev, int train, int B, int HW,
                   int C, int Cr, float eps, int relu, int dtype, float* part, float* rlnp, void* out, sde_stream_t stream);
/* Backward (mean and variance are detached): g = (d0 [+ d1 [+ d2]]) * relu'(out) (out needed when relu), stored in gm when gm != NULL (the
 * residual's gradient); dx = g * gamma * rstd; dgamma [Cr] (+)= sum g * xhat, dbeta [Cr] (+)= sum g (accumulate).  part as in forward.
 * Two launches. */
int sde_randln_bwd(const void* d0, const void* d1, const void* d2, const void* out, const void* y, const float* rlnp, const float* gamma, int relu, int B,
                   int HW, int C, int Cr, int dtype, float* part, float* dgamma, float* dbeta, int accumulate, void* gm, void* dx, sde_stream_t stream);
/* F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) of UpsampleBlock (L107-112): x [B,H,W,C] -> out [B,2H,2W,C] with torch's
 * source index scale = (H-1)/(2H-1).  Backward: dx [B,H,W,C], every input pixel gathers the output taps that read it. */
int sde_bilinear2_fwd(const void* x, int B, int H, int W, int C, int dtype, void* out, sde_stream_t stream);
int sde_bilinear2_bwd(const void* dout, int B, int H, int W, int C, int dtype, void* dx, sde_stream_t stream);
/* F.softplus(out_conv(x)) (L103; beta 1, threshold 20): channel 0 of y [B,H,W,ld] -> out [B,1,H,W] fp32, mirrored along x when flip.
 * Backward: dy [B,H,W,ld] = dout * sigmoid(y) (dout where y > 20) in channel 0, zero in the others. */
int sde_softplus_head_fwd(const void* y, int B, int H, int W, int ld, int flip, int dtype, float* out, sde_stream_t stream);
int sde_softplus_head_bwd(const void* y, const float* dout, int B, int H, int W, int ld, int flip, int dtype, void* dy, sde_stream_t stream);

/* GoogleResNetv2's up-sampling layer (csrc/deconv.hip; GoogleResNetv2.py:L42-44): y [B,2H,2W,ldy] = act(ConvTranspose2d(Cin, Cout, 3, stride 2,
 * padding 1, output_padding 1)(x) + bias) of x [B,H,W,C], split by output parity into four convolutions of the stored input (nine tap products per
 * input pixel; no zero-inserted image).  w_packed: [ldy][3][3][C], taps flipped -- with the ConvTranspose2d weight [Cin,Cout,3,3] read as the OIHW
 * weight of the adjoint Conv2d(Cout -> Cin, 3, stride 2, padding 1), sde_pack_weight(Cout = Cin, Cin = Cout, Cin_pad = ldy, Cout_pad = C, for_dgrad = 1);
 * the for_dgrad = 0 operand of the same call serves the layer's data gradient (a plain sde_conv_fwd of that adjoint) and sde_conv_wgrad of the
 * adjoint, with x as the "output gradient", its weight gradient.  act: SDE_ACT_NONE / SDE_ACT_ELU / SDE_ACT_RELU.  fp32 (the engine's fp32 MFMA
 * arithmetic) or bf16 storage (SDE_F16 is refused), fp32 accumulation; channels >= Cout of y are written as zeros. */
int sde_deconv3x3s2_fwd(const void* x, const void* w_packed, const float* bias, int act, int B, int H, int W, int C, int Cout, int ldy, int dtype,
                        void* y, sde_stream_t stream);

/* Grouped 3x3 convolution, the 3x3 of a ResNeXt bottleneck (csrc/gconv.hip): y [B,OH,OW,C] = conv(x [B,H,W,C]) with Cin == Cout == C, G groups,
 * padding 1, stride 1 or 2 (OH = (H - 1) / stride + 1), no bias, no activation.  C % 16 == 0 and C / G in {4, 8, 16, 32, 64}; fp32 or bf16 storage,
 * fp32 accumulation; any other argument is refused before a launch.  w: the fp32 MASTER weight, [C][C/G][3][3] or, with w_ohwi set, in the
 * trainer's channels-last order [C][3][3][C/G]: the kernels convert it on their way into LDS, there is no packed operand.  H, W are the sizes of x
 * (of dx for the data gradient) in every call.
 * stats (optional): [sde_gconv3x3_stats_rows + SDE_REDUCE_ROWS][C][2] per-workgroup (sum, sum of squares) of the stored outputs, the slab
 * sde_bn_finalize / sde_bn_finalize_apply read.  sde_gconv3x3_stats_rows: from the shape alone; -1 for an unsupported one.
 * sde_gconv3x3_wgrad: dw [C][C/G][3][3] (+)= the weight gradient; ws: sde_gconv3x3_wgrad_ws_bytes bytes of fp32 partials, summed in a fixed order
 * by a second launch (no atomics: bit-reproducible); flags: SDE_WREDUCE_ACCUMULATE | SDE_WREDUCE_OHWI, as sde_wreduce_item.accumulate. */
int sde_gconv3x3_stats_rows(int B, int H, int W, int C, int G, int stride, int dtype);
int sde_gconv3x3_fwd(const void* x, const float* w, int w_ohwi, int B, int H, int W, int C, int G, int stride, int dtype, void* y, float* stats,
                     sde_stream_t stream);
int sde_gconv3x3_dgrad(const void* dz, const float* w, int w_ohwi, int B, int H, int W, int C, int G, int stride, int dtype, void* dx,
                       sde_stream_t stream);
size_t sde_gconv3x3_wgrad_ws_bytes(int B, int H, int W, int C, int G, int stride, int dtype);
int sde_gconv3x3_wgrad(const void* x, const void* dz, int B, int H, int W, int C, int G, int stride, int dtype, float* ws, size_t ws_bytes, float* dw,
                       int flags, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * GoogleMotionNet / GooglePoseNet operators (csrc/motion.hip; detectron2/modeling/pose_net/GooglePoseNet.py), NHWC activations in fp32 or bf16
 * (SDE_F16 is refused), 16-byte channel groups.  The 3-channel motion field is fp32 [B,h,w,4] (channel 3 zero) in both modes.  No atomics:
 * repeated runs give identical bits.  No call synchronises.
 * ------------------------------------------------------------------------------------------------- */
/* MotionRefiner's input (L91-94): F.interpolate(field, (H, W), mode='bilinear', align_corners=True) for any size pair (source index
 * o * (h-1)/(H-1), 0 when H == 1) and cat([resized, skip], 1) in one pass.  skip [B,H,W,Cs], its first Cr channels real; X [B,H,W,Cx] in
 * `dtype`, Cx >= 3 + Cr, channels [resized (3), skip (Cr), zeros]; up [B,H,W,4] fp32 = the resized field.
 * Backward: g = dX0 [+ dX1] (either may be NULL); dfield [B,h,w,4] = the gather of g[..., 0:3] + dup (dup may be NULL) over the output
 * positions that read each field pixel; dskip [B,H,W,Cs] = g[..., 3:3+Cr], pad channels zero (NULL: not written). */
int sde_motion_resize_cat_fwd(const float* field, int h, int w, const void* skip, int B, int H, int W, int Cs, int Cr, int Cx, int dtype, void* X,
                              float* up, sde_stream_t stream);
int sde_motion_resize_cat_bwd(const void* dX0, const void* dX1, const float* dup, int B, int H, int W, int Cx, int Cr, int Cs, int h, int w, int dtype,
                              float* dfield, void* dskip, sde_stream_t stream);
/* MotionRefiner's tail (L95-99): out [P,4] fp32 = up [P,4] + w3 . cat[o1, o2] per pixel; o1, o2 [P,ld] with `mid` real channels each,
 * w3 [3][2*mid] fp32 (the bias-free 1x1 conv3, OIHW).  Backward: do1, do2 [P,ld] (pad channels zero), dw3 [3][2*mid] (overwritten) through
 * part [sde_motion_tail_blocks(P, ld, dtype)][3][2*mid] partial sums and a fixed-order final sum (two launches); d up = dout. */
int sde_motion_tail_fwd(const void* o1, const void* o2, const float* w3, const float* up, long P, int ld, int mid, int dtype, float* out,
                        sde_stream_t stream);
int sde_motion_tail_blocks(long P, int ld, int dtype);
int sde_motion_tail_bwd(const float* dout, const void* o1, const void* o2, const float* w3, long P, int ld, int mid, int dtype, void* do1, void* do2,
                        float* part, float* dw3, sde_stream_t stream);
/* GoogleMotionNet's head (L190-205): r = field * *scale; mask = 1: n = |r|_2 over the 3 channels, r *= (n > mean of n over all B*H*W pixels);
 * out [B,3,H,W] fp32 planar = r * *weight.  scale and weight are one-element device buffers (a captured graph follows later values).
 * part: [sde_motion_head_blocks(B*H*W)] floats; keep [B*H*W] bytes, the mask (both unused when mask = 0).  One launch, two with the mask.
 * Backward: g = dout * *weight * keep (keep NULL: all ones); dfield [B,H,W,4] = g * *scale; part[blk] = partial sums of sum g * field, whose
 * total is the gradient of *scale (the mask carries no gradient). */
int sde_motion_head_blocks(long P);
int sde_motion_head_fwd(const float* field, const float* scale, const float* weight, int mask, int B, int H, int W, float* part, unsigned char* keep,
                        float* out, sde_stream_t stream);
int sde_motion_head_bwd(const float* dout, const float* field, const float* scale, const float* weight, const unsigned char* keep, int B, int H, int W,
                        float* dfield, float* part, sde_stream_t stream);
/* Gradient of sde_prep_input without mean / std / flip: d0 [+ d1] [B,H,W,Cp] in `dtype` -> dimg [B,C,H,W] fp32 (d1 may be NULL). */
int sde_prep_input_bwd(const void* d0, const void* d1, int B, int C, int H, int W, int Cp, int dtype, float* dimg, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * PackNet's 3-D convolution (layers01.py:L223-298): x.unsqueeze(1) -> nn.Conv3d(1, 8, 3, padding=1) -> view(b, 8*D, h, w) on NHWC data:
 * y[b,h,w,f*D+ch] = bias[f] + sum w[f][kd][kh][kw] x[b,h+kh-1,w+kw-1,ch+kd-1].  w: [8][3][3][3] fp32 (torch's [8,1,3,3,3]), D % (16 B) == 0.
 * wgrad: part = workspace [sde_conv3d_wgrad_num_blocks()][224] floats; dw [8*27], dbias [8] (may be NULL). */
int sde_conv3d_fwd(const void* x, const float* w, const float* bias, int B, int H, int W, int D, int dtype, void* y, sde_stream_t stream);
int sde_conv3d_dgrad(const void* dy, const float* w, int B, int H, int W, int D, int dtype, void* dx, sde_stream_t stream);
int sde_conv3d_wgrad_num_blocks(int B, int H, int W, int D, int dtype);
int sde_conv3d_wgrad(const void* x, const void* dy, int B, int H, int W, int D, int dtype, float* part, float* dw, float* dbias, int accumulate,
                     sde_stream_t stream);

/* PackNet01's data movement (csrc/packnet.hip), NHWC, 16 bytes per lane, each other's backward:
 *   sde_space_to_depth: layers01.py:L138-160 `packing` (r = 2): x [B,H,W,C] -> y [B,H/2,W/2,4C], y[b,i,j,c*4+di*2+dj] = x[b,2i+di,2j+dj,c]
 *   sde_depth_to_space: nn.PixelShuffle(2) of layers01.py:L262-298:       x [B,H,W,C4] -> y [B,2H,2W,C4/4], the inverse permutation
 * sde_concat_fwd: PackNet01.py:L150-199 torch.cat([unpacked, skip(, nearest_x2(inv_depth))], 1) (version A) or [unpacked + skip(, ...)] (add = 1,
 * version B: C1 == C0) as ONE pass: out [B,H,W,Ct], Ct = channels used rounded up to the 16-byte group, fill = exact zeros; inv [B,H/2,W/2] fp32
 * or NULL.  sde_concat_bwd: d0 [B,H,W,C0] (add mode: also the gradient of p1), d1 [B,H,W,C1] (concat mode), d_inv [B,H/2,W/2] fp32 (2x2 sums) or NULL. */
int sde_space_to_depth(const void* x, int B, int H, int W, int C, int dtype, void* y, sde_stream_t stream);
int sde_depth_to_space(const void* x, int B, int H, int W, int C4, int dtype, void* y, sde_stream_t stream);
int sde_concat_fwd(const void* p0, const void* p1, const float* inv, int add, int B, int H, int W, int C0, int C1, int Ct, int dtype, void* out,
                   sde_stream_t stream);
int sde_concat_bwd(const void* dout, int add, int B, int H, int W, int C0, int C1, int Ct, int dtype, void* d0, void* d1, float* d_inv, sde_stream_t stream);
/* layers01.py:L105-133 InvDepth's tail + PackNet01.py:L120-123,L199 scale_inv_depth: logit = y[...,0] ([B,H,W,ld], the one-channel convolution's padded
 * output) -> inv [B,H,W] fp32 = sigmoid(logit) / min_depth_head (fed to the next decoder level) and depth [B,1,H,W] fp32 =
 * 1 / (1/max_depth + (1/min_depth - 1/max_depth) * inv), mirrored along x when flip.  Backward: d_inv and / or d_depth (either may be NULL) -> dy. */
int sde_inv_depth_head_fwd(const void* y, int B, int H, int W, int ld, float min_depth_head, float min_depth, float max_depth, int flip, int dtype, float* inv,
                           float* depth, sde_stream_t stream);
int sde_inv_depth_head_bwd(const void* y, const float* d_inv, const float* d_depth, int B, int H, int W, int ld, float min_depth_head, float min_depth,
                           float max_depth, int flip, int dtype, void* dy, sde_stream_t stream);

/* torch.optim.Adam / AdamW step (projects/MonoDepth2/train.py:L50-57, projects/Supervised/train.py:L77-81) over ONE flat fp32 buffer.
 * The descriptor is HOST memory and is copied into the kernel arguments (nothing to upload or keep alive): segment s covers
 * [seg_end[s-1], seg_end[s]) with its own lr / weight decay; bias_corr1/2 = (1 - beta1^t, 1 - beta2^t) (the step count lives on the host);
 * grad_scale multiplies g first (1/world_size after a sum all-reduce).
 * scale_state (optional, DEVICE float[4] = {loss_scale, found_inf, growth_tracker, applied_steps}): fp16 training with dynamic loss
 * scaling, the GradScaler of the reference's AMPTrainer (detectron2/engine/train_loop.py:L294-341) without its host sync:
 * sde_grad_check raises found_inf when any gradient is inf / nan, sde_adam_step divides the gradients by loss_scale and SKIPS the whole
 * update when found_inf is set, sde_loss_scale_update then backs the scale off (x backoff_factor) or counts towards growth (x
 * growth_factor every growth_interval clean steps), counts the step in applied_steps when it was NOT skipped, and clears found_inf.
 * With scale_state the optimizer's step count lives on the device (GradScaler.step skips optimizer.step(), so Adam's `step` does not
 * advance on an overflow): the kernel ignores bias_corr1/2 and forms 1 - beta^(applied_steps + 1) itself from beta1_d / beta2_d.
 * The loss is multiplied by scale_state[0] on the device before backward.
 * clip_state (optional, DEVICE float[2] = {total_norm, clip_coef}; NULL: off, the update is what it is without the field): gradient-norm
 * clipping, torch.nn.utils.clip_grad_norm_(model.parameters(), SOLVER.CLIP_GRAD) of projects/MotionLearning/train.py:L157 without its per-tensor
 * norms and without rescaling the gradient in memory: sde_grad_norm reads the flat gradient once (4 * n bytes) and leaves
 * total_norm = grad_scale * ||g||_2 (the norm of the averaged gradient) and clip_coef = min(1, max_norm / (total_norm + 1e-6)) on the device;
 * sde_adam_step multiplies grad_scale by clip_coef.  A NaN norm gives a NaN coefficient and NaN parameters, an infinite one the coefficient 0,
 * both as in torch.  work: DEVICE float[SDE_GRAD_NORM_WORK], one partial sum per workgroup; no atomics, a fixed summation order: two calls on
 * the same buffer give the same bits. */
#define SDE_ADAM_MAX_SEG 8
#define SDE_GRAD_NORM_WORK 1024
typedef struct sde_adam_desc {
    long seg_end[SDE_ADAM_MAX_SEG];
    float seg_lr[SDE_ADAM_MAX_SEG], seg_wd[SDE_ADAM_MAX_SEG];
    int32_t nseg, decoupled_wd;
    float beta1, beta2, eps, bias_corr1, bias_corr2, grad_scale;
    const float* scale_state;
    double beta1_d, beta2_d;       /* the betas in double (device-side bias corrections of the scale_state path) */
    const float* clip_state;
} sde_adam_desc;
int sde_adam_step(float* p, const float* g, float* m, float* v, long n, const sde_adam_desc* d, sde_stream_t stream);
/* The same update (p, m, v come out bit-identical to sde_adam_step) that also writes twin[i] = (twin_dtype) p_new[i] for every i < n, with the
 * conversion of the weight pack: twin is a DEVICE buffer of n SDE_BF16 / SDE_F16 elements in the flat order of p.  Where a convolution weight sits
 * in p channels-last without channel padding, its slot of the twin IS the packed forward operand (sde_pack_item: SDE_W_TWIN16 builds the
 * data-gradient operand from it).  A step skipped through scale_state leaves the twin untouched, like p.  p, g, m, v 16-byte aligned, twin 8-byte. */
int sde_adam_step_twin(float* p, const float* g, float* m, float* v, long n, const sde_adam_desc* d, void* twin, int twin_dtype, sde_stream_t stream);
int sde_grad_check(const float* g, long n, float* scale_state, sde_stream_t stream);
int sde_grad_norm(const float* g, long n, float* work, float* clip_state, float grad_scale, float max_norm, sde_stream_t stream);
int sde_loss_scale_update(float* scale_state, float growth_factor, float backoff_factor, int growth_interval, sde_stream_t stream);


/* ---------------------------------------------------------------------------------------------------
 * Device-side input pipeline: N uint8 frames [N][Hs][Ws][3] of ONE source size -> the resized (h x w), colour-jittered frame and
 * the resized un-jittered frame as fp32 NCHW in [0, 1] (`img` / `img_orig`, `ctx_img` / `ctx_img_orig` of the batch dict), replacing the CPU chain
 * Resize -> RandomImageAug -> ToTensor of detectron2/data/preprocess/augmentation.py:L124-166,L229-266 for the image entries, in the same integer /
 * float32 arithmetic (OpenCV's fixed-point INTER_LINEAR; Pillow's Image.blend / L / HSV conversions), i.e. bit-identical to this package's CPU chain.
 * xtab [w][4] = (x0, x1, a0, a1), ytab [h][4] = (y0, y1, b0, b1): OpenCV's source taps and 11-bit weights per output column / row (device, 16-byte
 * aligned; data/device_aug.py builds them once per size pair).  jit [N][8] (device): brightness, contrast, saturation, hue factor, then the order of
 * the four steps (0 brightness, 1 contrast, 2 saturation, 3 hue) as floats; jit[n][4] < 0: frame n is not jittered.  lsum [N]: workspace.
 * orig may be NULL.  Two launches (the contrast step needs the frame's mean luminance at that point of the chain), no host synchronisation. */
int sde_image_prep_u8(const uint8_t* src, int N, int Hs, int Ws, int h, int w, const int* xtab, const int* ytab, const float* jit, unsigned* lsum, float* img,
                      float* orig, sde_stream_t stream);
/* G <= 4 frame tensors of one shape and one parameter set per sample (a MonoDepth2 batch: target frames + context frames) in ONE pair of launches:
 * src / img / orig are HOST arrays of G device pointers (orig NULL: none), lsum [G*N]. */
int sde_image_prep_u8_multi(const uint8_t* const* src, int G, int N, int Hs, int Ws, int h, int w, const int* xtab, const int* ytab, const float* jit, unsigned* lsum,
                            float* const* img, float* const* orig, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Evaluation: detectron2/evaluation/depth_evaluation.py:L74-104 kitti_evaluator.process for ONE image, with
 * compute_errors (L30-53), garg_crop / eigen_crop (L16-27, as the window [y0,y1) x [x0,x1) in gt coordinates), the 1e-3 < gt < 80 median
 * scaling of TEST.GT_SCALE (L91-93) and the postprocess.backward() chain folded into two index maps: ymap[gh], xmap[gw] give the
 * prediction row / column every ground-truth row / column reads (Resize.backward = cv2 INTER_NEAREST, augmentation.py:L163-166; the crop
 * un-pastes of L67-74, L113-120; -1 = outside the prediction: value 0).  pred [ph,pw], gt [gh,gw] fp32, maps int32, all device memory.
 * part: workspace [sde_depth_metrics_num_blocks(y1-y0, x1-x0)][SDE_EVAL_NSUM] doubles; med: workspace of 4 x 4 bytes, ZEROED by the caller;
 * keys: workspace of 2 * (y1-y0) * (x1-x0) uint32 for the median selection (needed only when gt_scale == 1).
 * gt_scale: 0 = no scaling; 1 = compute the medians into med[0..1], then scale; 2 = med[0..1] already hold the medians of this image and
 * window (the evaluators of one config share them: same mask, same crop).
 * out[12] doubles = silog, log10, abs_rel, sq_rel, rms, log_rms, d1, d2, d3 (compute_errors' return order), then the number of valid pixels
 * (0: the reference skips the image, L102), median(gt), median(pred) (0 when gt_scale == 0).  No host synchronisation. */
#define SDE_EVAL_NSUM 11
int sde_depth_metrics_num_blocks(int crop_h, int crop_w);
int sde_depth_metrics(const float* pred, int ph, int pw, const float* gt, int gh, int gw, const int* ymap, const int* xmap, int y0, int y1,
                      int x0, int x1, float min_depth, float max_depth, int gt_scale, double* part, float* med, unsigned* keys, double* out,
                      sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Presentation (csrc/present.hip; binding in hip/present.py): N network outputs pred [N,ph,pw] fp32 of ONE source size -> what tools/demo.py
 * shows and saves, in one launch.  ymap [H] / xmap [W] are the maps of sde_depth_metrics (restored pixel -> prediction pixel, -1 = outside:
 * value 0); the kernel indexes pred with whatever they hold, so the caller validates them ([-1, ph) / [-1, pw)).  For every restored pixel d:
 *   depth_full [N,H,W] fp32 = d                                   (optional, NULL skips it: the postprocess.backward() chain of the reference);
 *   depth_u16  [N,H,W] uint16 = (uint16)(d * 255), fp32 product truncated, clamped to [0, 65535], NaN -> 0   (optional: write_depth's format);
 *   colour = lut[min(255, (int)(powf(d, gamma) / powf(vmax, gamma) * 256))], NaN and d < 0 as d = 0, lut [256][3] uint8 (demo.py:L77).
 * canvas [N][2H][W][3] uint8 with frame [N,H,W,3] uint8 (RGB) non-NULL: rows [0, H) the frame, rows [H, 2H) the colours (demo.py:L100-104);
 * frame == NULL: canvas [N][H][W][3] holds the colours only.  No pointer needs more than its element's alignment.
 * Refused before any launch: N, H, W, ph, pw <= 0, vmax <= 0, gamma <= 0, NULL pred / maps / lut / canvas.  No host synchronisation, no
 * allocation, no atomics. */
int sde_depth_present(const float* pred, int N, int ph, int pw, const int* ymap, const int* xmap, int H, int W, float vmax, float gamma,
                      const uint8_t* lut, const uint8_t* frame, float* depth_full, uint16_t* depth_u16, uint8_t* canvas, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Point clouds (csrc/cloud.hip; binding in hip/cloud.py): back-projection of depth, detectron2/geometry/camera.py:L25-37 and L125-138.
 *
 * sde_depth_cloud: N network outputs pred [N,ph,pw] fp32 of ONE source size -> per frame a compacted list of coloured points at the restored
 * size.  ymap [H] / xmap [W]: the maps of sde_depth_present, same contract (-1 = outside: value 0; the caller validates the ranges).
 * frame [N,H,W,3] uint8 RGB or NULL (colour 255,255,255).  K [N,3,3] fp32, intrinsics at the restored (source) size, metres out for metres in;
 * only fx = K[0], cx = K[2], fy = K[4], cy = K[5] are read.  Candidates are the pixels with v % step == 0 && u % step == 0, in raster order.
 * With d the restored depth of pixel (u, v): the pixel is kept iff d is finite and min_depth < d <= max_depth (fp32 comparisons on the stored
 * value).  A kept pixel gives one 16-byte record { float x, y, z; uint8 r, g, b, a }, written by one aligned 16-byte store, evaluated in fp32
 * in exactly this order, nothing fused:
 *   Kinv00 = 1 / fx;  Kinv11 = 1 / fy;  Kinv02 = (-1 * cx) / fx;  Kinv12 = (-1 * cy) / fy;          (inv_intrinsics)
 *   x = d * (Kinv00 * (float)u + Kinv02);   y = d * (Kinv11 * (float)v + Kinv12);   z = d;   a = 255.
 * points [N][cap][16 bytes] with cap = sde_depth_cloud_capacity(H, W, step) = ceil(H / step) * ceil(W / step), 16-byte aligned; count [N]
 * int32, device memory.  The records of frame n fill [0, count[n]) of its cap slots in raster order; the bytes behind them are not touched.
 * workspace: sde_depth_cloud_ws_bytes(N, H, W, step) bytes of device memory, 4-byte aligned, contents irrelevant (both queries return 0 for
 * sizes the entry point refuses).  Three launches ordered on the stream (counts per workgroup, exclusive scan, scatter); no workgroup waits
 * for another, no atomics, no host synchronisation, no allocation: legal under graph capture, the same bytes every run.
 * Refused before any launch: N, H, W, ph, pw <= 0, step < 1, min_depth >= max_depth (or a NaN), NULL pred / maps / K / points / count,
 * points off a 16-byte boundary, a workspace that is NULL or smaller than the query reports.
 *
 * sde_img_to_points_fwd / _bwd: img_to_points(depth [B,1,H,W], R [B,3,3], t), fp32, planar.  t [B,3] (t_per_pixel == 0) or [B,3,H*W] (!= 0).
 *   points [B,3,H,W]: points_c = R_c0 * (u * d) + R_c1 * (v * d) + R_c2 * d + t_c           (u = column, v = row)
 * Backward from grad [B,3,H,W]: ddepth [B,H,W] = sum_c grad_c * (R_c0 * u + R_c1 * v + R_c2); dR [B,3,3] = sum_p grad_p (x) (d_p * [u,v,1]);
 * dt [B,3] = sum_p grad_p (NULL skips it: with a per-pixel t the gradient of t is grad itself; dR NULL skips it too, and with both NULL the second
 * launch and the sums are left out and part may be NULL).  part: workspace of
 * B * sde_img_to_points_num_blocks(H, W) * 12 floats; the twelve sums of a sample are per-workgroup fp32 partials added in workgroup order in
 * fp64 by a second launch.  Refused before any launch: B, H, W <= 0, NULL depth / R / t / points (fwd), NULL grad / depth / R / ddepth, or dR / dt
 * without part (bwd).  No atomics, no host synchronisation. */
long sde_depth_cloud_capacity(int H, int W, int step);
size_t sde_depth_cloud_ws_bytes(int N, int H, int W, int step);
int sde_depth_cloud(const float* pred, int N, int ph, int pw, const int* ymap, const int* xmap, int H, int W, const uint8_t* frame, const float* K,
                    float min_depth, float max_depth, int step, void* workspace, size_t workspace_bytes, void* points, int* count,
                    sde_stream_t stream);
int sde_img_to_points_num_blocks(int H, int W);
int sde_img_to_points_fwd(const float* depth, const float* R, const float* t, int t_per_pixel, int B, int H, int W, float* points,
                          sde_stream_t stream);
int sde_img_to_points_bwd(const float* grad, const float* depth, const float* R, int B, int H, int W, float* part, float* ddepth, float* dR, float* dt,
                          sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Raw LiDAR scans -> sparse depth maps (csrc/lidar.hip; binding and host twin in hip/lidar.py): the inverse of the point clouds above, and the
 * routine that wrote the proj_depth/velodyne caches of the Eigen split (generate_depth_map of monodepth2 / packnet-sfm).
 *
 * pts [B][cap][stride] fp32, stride 3 or 4, only x, y, z are read; count [B] int32 in device memory, 0 <= count[b] <= cap, rows behind count[b]
 * are never read (a count above cap is treated as cap).  proj [B][3][4] fp32 row-major: the whole scanner-to-image matrix (KITTI: P_rect_0c *
 * R_rect_00 * Tr_velo_to_cam).  origin [B][2] int32 (x0, y0): the top-left corner, in full-image pixels, of the H x W window that is written.
 * depth [B][H][W] fp32: EVERY element is written, 0 where no point lands.  Per point, in fp32, in exactly this order, nothing fused:
 *   u = m00 * x + m01 * y + m02 * z + m03;   v, w likewise from rows 1 and 2;   d = w, or x with SDE_LIDAR_VEL_DEPTH;
 *   kept iff x, y, z are finite, w > 0, 0 < d < inf, and (SDE_LIDAR_FRONT_ONLY) x >= 0;
 *   px = (int)rintf(u / w) - 1 - x0;   py = (int)rintf(v / w) - 1 - y0        (round-half-even; - 1: the routine's 1-based pixel convention);
 *   kept iff 0 <= px < W and 0 <= py < H (and |rintf(.)| < 1e9, so that the conversion is defined).
 * The smallest d that reaches a pixel wins it (integer atomicMin on the bit pattern: order-independent, bit-reproducible); min(d, max_depth) is
 * applied when the map is finalised, max_depth <= 0 (or NaN): no clipping.
 * Deviation from the published routine: w > 0 and d > 0.  The routine lets a point behind the image plane project mirrored into the image and
 * take the pixel with a negative depth, and zeroes that pixel at the end (depth[depth < 0] = 0), hiding whatever positive depth lay there;
 * with its x >= 0 pre-filter and a forward camera that needs a point less than the camera offset in front of the scanner.  Here such a point
 * is dropped and the pixel keeps its closest positive depth.
 * Three launches ordered on the stream (fill, scatter, finalise), each one grid-stride grid over all B; no host synchronisation, no allocation,
 * no workspace: legal under graph capture.  Refused before any launch: stride not 3 or 4, H, W or cap <= 0, B < 0, unknown flag bits, a NULL
 * pointer with B > 0.  B == 0 returns 0 and launches nothing. */
#define SDE_LIDAR_VEL_DEPTH 1
#define SDE_LIDAR_FRONT_ONLY 2
int sde_lidar_depth(const float* pts, int cap, int stride, const int* count, int B, const float* proj, const int* origin, int H, int W,
                    int flags, float max_depth, float* depth, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Optical flow between two frames from depth and relative pose (csrc/flow.hip; binding in hip/flow.py): img_to_points into points_to_img,
 * detectron2/geometry/camera.py:L125-163, for N predictions of ONE source size in one launch.
 *
 * pred [N,ph,pw] fp32: the depth of frame A at the network's size.  ymap [H] / xmap [W]: the maps of sde_depth_present, same contract (-1 =
 * outside: value 0; the caller validates the ranges).  K [N,3,3] fp32, intrinsics at the restored (source) size; only fx = K[0], cx = K[2],
 * fy = K[4], cy = K[5] are read.  T [N,4,4] fp32 row-major, the pose A -> B: with R = T[:3,:3], t = T[:3,3], p_B = R p_A + t (only those twelve
 * entries are read).  motion [N,3,ph,pw] fp32 or NULL: a per-pixel translation added to t, read through the same maps, 0 outside them; NULL
 * gives the rigid (ego-motion) flow.  For the restored pixel (u, v), u = column, v = row, with d its restored depth and m its restored motion,
 * evaluated in fp32 in exactly this order, nothing fused (every division and the square root correctly rounded):
 *   Kinv00 = 1 / fx;  Kinv11 = 1 / fy;  Kinv02 = (-1 * cx) / fx;  Kinv12 = (-1 * cy) / fy;                       (sde_depth_cloud's)
 *   px = d * (Kinv00 * (float)u + Kinv02);   py = d * (Kinv11 * (float)v + Kinv12);   pz = d;
 *   s_r = t_r + m_r;   q_r = ((R_r0 * px + R_r1 * py) + R_r2 * pz) + s_r                                          for the rows r = x, y, z;
 *   nx = fx * qx + cx * qz;   ny = fy * qy + cy * qz;   den = qz + 1e-6f;   X = nx / den;   Y = ny / den;
 *   valid bit 0 (value 1): the pixel is inside both maps, d is finite and > 0, qz > 0, X and Y are finite;
 *   valid bit 1 (value 2): bit 0 and 0 <= X < (float)(W - 1) and 0 <= Y < (float)(H - 1)         (the reference's valid_proj_mask, L154-156);
 *   flow = (X - (float)u, Y - (float)v) where bit 0 is set, else (0, 0).
 * Outputs, device memory, each optional (NULL skips it) but at least one: flow [N,H,W,2] fp32 in pixels of the restored size, valid [N,H,W]
 * uint8, and canvas, the flow in the colours of the wheel [ncols][3] uint8 (the Middlebury wheel has 55 entries; hip/flow.py builds it).  With
 * (fx, fy) the flow of a pixel with bit 0, in fp32:
 *   fu = fx / max_flow;  fv = fy / max_flow;  rad = min(1, sqrtf(fu * fu + fv * fv));
 *   a = atan2f(-fv, -fu) / (float)pi;   fk = (a + 1) * 0.5f * (float)(ncols - 1);   k0 = (int)fk clamped to [0, ncols - 1];
 *   k1 = k0 + 1, or 0 when that is ncols;   f = fk - (float)k0;
 *   per channel, c0 = wheel[k0][ch] / 255.f and c1 = wheel[k1][ch] / 255.f:   col = (1 - f) * c0 + f * c1;   col = 1 - rad * (1 - col);
 *   byte = (uint8)(255.f * col), truncated, clamped to [0, 255]                    (zero flow is white, |flow| >= max_flow the pure wheel colour).
 * Pixels without bit 0 are black.  canvas [N][2H][W][3] with frame [N,H,W,3] uint8 (RGB) non-NULL: rows [0, H) the frame, rows [H, 2H) the
 * colours, as sde_depth_present stacks them; frame == NULL: canvas [N][H][W][3] holds the colours only (frame is ignored without a canvas).
 * No pointer needs more than its element's alignment.  One launch, no atomics, no workspace, no host synchronisation, no allocation: legal
 * under graph capture, the same bytes every run.  Refused before any launch: N, H, W, ph, pw <= 0, max_flow <= 0 (or a NaN), ncols <= 0 or
 * > 256, NULL pred / maps / K / T, all three outputs NULL, a canvas without a wheel. */
int sde_pair_flow(const float* pred, int N, int ph, int pw, const int* ymap, const int* xmap, int H, int W, const float* K, const float* T,
                  const float* motion, const uint8_t* wheel, int ncols, float max_flow, const uint8_t* frame, float* flow, uint8_t* valid,
                  uint8_t* canvas, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Temporally fused depth for frame sequences (csrc/temporal.hip; binding and host twin in hip/temporal.py): the previous frame's depth is
 * forward-projected into the current camera, overlaps are resolved by a z-buffer, and the result is blended with the current prediction
 * where the two agree.  No counterpart in the reference.
 *
 * prev, cur [N,h,w] fp32: the previous frame's (fused) depth and the current prediction, both at the network's size.  K [N,3,3] fp32, the
 * intrinsics AT THAT SIZE; only fx = K[0], cx = K[2], fy = K[4], cy = K[5] are read.  T [N,4,4] fp32 row-major, the pose previous -> current:
 * with R = T[:3,:3], t = T[:3,3], p_cur = R p_prev + t (only those twelve entries are read).  motion [N,3,h,w] fp32 or NULL: a per-pixel
 * translation on the PREVIOUS frame's grid, added to t.  zbuf [N,h,w] uint32: workspace, every element is overwritten.  alpha in [0, 1): the
 * weight of the warped depth in the blend; tol > 0: the relative difference up to which the two depths count as the same surface.
 * Three launches ordered on the stream, each one grid-stride grid over all N:
 *   fill     every zbuf element <- 0x7f800000 (+inf).
 *   scatter  for the previous frame's pixel (u, v), u = column, v = row, d = prev[n,v,u], m its motion (0 with motion == NULL), in fp32 in
 *            exactly the operation order of sde_pair_flow above, nothing fused:
 *              Kinv00 = 1 / fx;  Kinv11 = 1 / fy;  Kinv02 = (-1 * cx) / fx;  Kinv12 = (-1 * cy) / fy;
 *              px = d * (Kinv00 * (float)u + Kinv02);   py = d * (Kinv11 * (float)v + Kinv12);   pz = d;
 *              s_r = t_r + m_r;   q_r = ((R_r0 * px + R_r1 * py) + R_r2 * pz) + s_r                               for the rows r = x, y, z;
 *              nx = fx * qx + cx * qz;   ny = fy * qy + cy * qz;   den = qz + 1e-6f;   X = nx / den;   Y = ny / den;
 *            kept iff d is finite and > 0, qz > 0, qz is finite, X and Y are finite;  rx = rintf(X), ry = rintf(Y) (round-half-even), kept iff
 *            |rx|, |ry| < 1e9f (so that the conversion is defined) and 0 <= rx < w, 0 <= ry < h;  then ONE no-return
 *            atomicMin(zbuf[n,ry,rx], bits of qz).  Positive finite floats order like their bit patterns and a minimum does not depend on
 *            the order of arrival: the same bytes every run.
 *   fuse     for the current frame's pixel i:  z = zbuf[i];  if z is empty (+inf), z = the unsigned minimum of the non-empty entries among
 *            the up to eight neighbours inside the image, and, if there is one, the pixel is FILLED;  if z is still empty the pixel is a hole.
 *              wv = hole ? 0 : float(z);   c = cur[i];   c_ok = c finite and > 0;
 *              diff = wv - c;   lim = tol * fminf(wv, c);   consistent = !hole && c_ok && fabsf(diff) <= lim;
 *              fused[i] = consistent ? c + alpha * diff : c;
 *              state[i] bits 0-1: 0 NEW (a hole, or c not usable), 1 FUSED (consistent), 2 NEARER (inconsistent, diff < 0: the warped surface
 *              lies in front of the prediction), 3 FARTHER (inconsistent, diff > 0);  bit 2 (value 4): FILLED;
 *              warped[i] = wv.
 * fused [N,h,w] fp32 is always written and may alias prev and / or cur (a state buffer updated in place); state [N,h,w] uint8 and warped
 * [N,h,w] fp32 may each be NULL.  A prev of zeros scatters nothing: fused == cur and state == 0 everywhere, the first frame of a sequence.
 * The splat is nearest-pixel and the hole filling one ring wide; alpha is fixed and the warped depth is not re-aligned in scale.
 * No allocation, no host synchronisation, no workspace besides zbuf: legal under graph capture.  Refused before any launch: N, h or w <= 0,
 * alpha outside [0, 1) (or a NaN), tol <= 0 (or a NaN), NULL prev / cur / K / T / zbuf / fused. */
#define SDE_TEMPORAL_NEW 0
#define SDE_TEMPORAL_FUSED 1
#define SDE_TEMPORAL_NEARER 2
#define SDE_TEMPORAL_FARTHER 3
#define SDE_TEMPORAL_FILLED 4
int sde_depth_warp_fuse(const float* prev, const float* cur, const float* K, const float* T, const float* motion, int N, int h, int w,
                        float alpha, float tol, uint32_t* zbuf, float* fused, uint8_t* state, float* warped, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * A sequence's depth fused into one truncated-signed-distance (TSDF) volume (csrc/volume.hip; binding and host twins in hip/volume.py): every
 * frame's depth is averaged into a voxel grid through its world-to-camera pose, and the zero crossings of the grid are the surface.  No
 * counterpart in the reference.
 *
 * The volume: nx x ny x nz voxels, x fastest, linear index v = (k * ny + j) * nx + i; every dimension in [1, 1024], nx * ny * nz <= 2^30.
 * Three device arrays: tsdf [nz,ny,nx] fp32, weight [nz,ny,nx] fp32, rgba [nz,ny,nx,4] uint8 (4-byte aligned; NULL: no colour).  A fresh volume
 * is tsdf = 1, weight = 0, rgba = 0, written by the caller.  origin [3]: HOST memory, the corner of voxel (0,0,0) in world coordinates, read
 * before the launch; voxel: the edge length.  The centre of voxel (i,j,k), in fp32, nothing fused:
 *   wx = ox + ((float)i + 0.5f) * voxel;   wy = oy + ((float)j + 0.5f) * voxel;   wz = oz + ((float)k + 0.5f) * voxel.
 *
 * sde_pose_compose: C <- T * C for ONE rigid 4x4 fp32 transform, both row-major in device memory, in place.  For the rows r = 0, 1, 2:
 *   C'_rc = (T_r0 * C_0c + T_r1 * C_1c) + T_r2 * C_2c          for c = 0, 1, 2;      C'_r3 = ((T_r0 * C_03 + T_r1 * C_13) + T_r2 * C_23) + T_r3;
 * the bottom row is written as 0 0 0 1 (those of T and C are not read).  With C the world-to-camera pose of frame i (p_cam = C p_world, the
 * first frame as the world: C_0 = I) and T_i the step i -> i+1 (p_{i+1} = T_i p_i, what the pose network predicts), C_{i+1} = T_i C_i: the
 * inverse of the camera-to-world chain of accumulate_poses, and no inversion on the device.  One launch of one workgroup.  Refused: NULL T or C.
 *
 * sde_tsdf_integrate: ONE frame into the volume.  pred [ph,pw] fp32, ymap [H] / xmap [W] (the maps of sde_depth_present, same contract: -1 =
 * outside; the caller validates the ranges), frame [H,W,3] uint8 RGB or NULL, K [3,3] fp32 at the restored (source) size (only fx = K[0],
 * cx = K[2], fy = K[4], cy = K[5] are read), C [4,4] fp32 in device memory, world -> camera (only its top three rows are read).  For the voxel
 * (i,j,k) with centre (wx,wy,wz), in fp32 in exactly this order, nothing fused (every division correctly rounded):
 *   1. q_r = ((C_r0 * wx + C_r1 * wy) + C_r2 * wz) + C_r3  for the rows r = x, y, z;                       kept iff qz is finite and > 0;
 *   2. nx = fx * qx + cx * qz;  ny = fy * qy + cy * qz;  den = qz + 1e-6f;  X = nx / den;  Y = ny / den;       (sde_pair_flow's projection)
 *      rx = rintf(X), ry = rintf(Y) (round-half-even);      kept iff |rx|, |ry| < 1e9f and, with ix = (int)rx, iy = (int)ry, 0 <= ix < W, 0 <= iy < H;
 *   3. my = ymap[iy];  mx = xmap[ix];                                                                         kept iff both >= 0;
 *   4. d = pred[my * pw + mx];                              kept iff d is finite and min_depth < d <= max_depth  (sde_depth_cloud's rule);
 *   5. sdf = d - qz;                                                                                          kept iff sdf >= -trunc;
 *   6. t = fminf(1.f, sdf / trunc);   w0 = weight[v];   t0 = tsdf[v];
 *      tsdf[v] = (t0 * w0 + t) / (w0 + 1.f);   weight[v] = fminf(w0 + 1.f, max_weight);
 *   7. with frame and rgba both non-NULL, and only where sdf <= trunc: per channel, with c0 the stored byte and f the frame's at (iy, ix),
 *      c = ((float)c0 * w0 + (float)f) / (w0 + 1.f), stored as (uint8)(c + 0.5f); the alpha byte becomes 255.
 * A voxel that is not kept is neither read from nor written to the three arrays.  Voxels are independent: one launch (a grid-stride grid), no
 * atomics, no workspace, no allocation, no host synchronisation: legal under graph capture, the same bytes every run.  frame without rgba and
 * rgba without frame are allowed: colour is skipped.  Refused before any launch: H, W, ph, pw <= 0, dims outside the limits above, voxel, trunc
 * or max_weight <= 0 (or a NaN), min_depth >= max_depth (or a NaN), NULL pred / maps / K / C / origin / tsdf / weight, rgba off a 4-byte boundary.
 *
 * sde_tsdf_points: the zero crossings of the volume as the 16-byte records { float x, y, z; uint8 r, g, b, a } of sde_depth_cloud, each written
 * by one aligned 16-byte store.  A voxel is valid iff weight >= min_weight (min_weight >= 1).  For the voxel v and, in the order x, y, z, its +1
 * neighbour n along that axis inside the grid: one record iff both are valid and (tsdf[v] < 0) != (tsdf[n] < 0).  With tv = tsdf[v], tn = tsdf[n]:
 *   f = tv / (tv - tn);   the coordinate along the axis = (the centre of v along it) + f * voxel;   the other two are the centre's;
 *   colour: rgba[v] if f < 0.5f, else rgba[n] (0, 0, 0 with rgba == NULL);   a = 255.
 * Record order: ascending v, then axis.  points [cap][16 bytes], 16-byte aligned; count [1] int32: the total number of crossings, also when it
 * exceeds cap (saturated at 2^31 - 1); records at positions >= cap are not written, and the bytes behind the written records are not touched.
 * workspace: sde_tsdf_points_ws_bytes(nx, ny, nz) bytes of device memory, 4-byte aligned, contents irrelevant (0 for dims the entry points
 * refuse).  Three launches ordered on the stream (crossings per tile of 256 voxels, exclusive scan, scatter); no workgroup waits for another, no
 * atomics, no host synchronisation, no allocation: legal under graph capture, the same bytes every run.  Refused before any launch: dims outside
 * the limits, voxel <= 0, min_weight < 1 (or a NaN), cap outside [1, 2^31), NULL tsdf / weight / origin / points / count, points off a 16-byte
 * or rgba off a 4-byte boundary, a workspace that is NULL or smaller than the query reports.
 *
 * sde_tsdf_mesh: the surface as a triangle mesh by surface nets (no case table): ONE vertex per cell that holds a crossing, ONE quad (two
 * triangles) per crossing edge -- the connectivity of the records of sde_tsdf_points.  A crossing edge (v, a) is exactly a record of
 * sde_tsdf_points: the same validity (weight >= min_weight), the same sign rule, the same point (f, centre + f * voxel) and the same colour.
 * Cell (i,j,k), i < nx-1, j < ny-1, k < nz-1, is named by its lowest corner and has the linear index of that voxel.  Its 12 edges in order:
 * axis x, y, z; within an axis, with b < c the other two axes, the edge starts at the corner offset (db, dc) = (0,0), (1,0), (0,1), (1,1).
 * A cell has a vertex iff m >= 1 of its edges cross.  The vertex is one 16-byte record { float x, y, z; uint8 r, g, b, a } (sde_depth_cloud's):
 *   each coordinate: s = 0.f;  s = s + (the crossing point's coordinate) over the m crossing edges in edge order;  stored s / (float)m;  nothing fused;
 *   each colour channel: the integer sum t of the m crossings' bytes, stored (uint8)((float)t / (float)m + 0.5f);   a = 255;   0, 0, 0 with rgba == NULL.
 * Vertices are numbered from 0 in ascending cell index.  A crossing edge (v, a), v = (i,j,k), gives two triangles iff the four cells around it
 * exist: v's coordinates along b and c lie in [1, n_b - 2] and [1, n_c - 2].  With q0..q3 the vertex numbers of the cells at the offsets (-1,-1),
 * (0,-1), (0,0), (-1,0) in (b, c) from v, the quad is q0 q1 q2 q3 when (tsdf[v] < 0) != (a == y), else q0 q3 q2 q1 ((y, x, z) is left-handed);
 * the triangles are (p0, p1, p2) and (p0, p2, p3) of the quad p.  Normals point from negative to positive tsdf: towards the camera that saw the
 * surface.  faces [cap_faces][3] int32, 4-byte aligned: ascending v, then axis, the two triangles of a quad next to each other.
 * vertices [cap_vertices][16 bytes], 16-byte aligned.  count [2] int32: count[0] the number of vertices, count[1] the number of triangles, also
 * when they exceed the caps (each saturated at 2^31 - 1).  Records and triangles at positions >= their cap are not written, the bytes behind the
 * written ones are not touched; a written triangle always holds the true vertex numbers, also those >= cap_vertices: with count[0] >
 * cap_vertices the mesh is incomplete and the caller runs again with more room.  A grid with a dimension of 1 has no cells: both counts are 0.
 * workspace: sde_tsdf_mesh_ws_bytes(nx, ny, nz) bytes of device memory (0 for dims the entry points refuse), 4-byte aligned, CONTENTS IRRELEVANT
 * on entry: two counts per tile of 256 voxels and a cell -> vertex number map of 4 B per voxel, which is written for every cell that has a vertex
 * and read only for such cells.  Four launches ordered on the stream (both counts per tile, one scan of both lists, vertices + map, faces); no
 * workgroup waits for another, no atomics, no host synchronisation, no allocation: legal under graph capture, the same bytes every run.  Refused
 * before any launch: dims outside the limits, voxel <= 0, min_weight < 1 (or a NaN), either cap outside [1, 2^31), NULL tsdf / weight / origin /
 * vertices / faces / count, vertices off a 16-byte or faces / rgba off a 4-byte boundary, a workspace that is NULL, misaligned or too small.
 *
 * sde_tsdf_render: the volume seen from a camera, by ray casting: ONE launch renders ONE picture of H x W pixels from the arrays as they are.
 * K [3,3] fp32 (fx = K[0], cx = K[2], fy = K[4], cy = K[5] are read) and C [4,4] fp32, world -> camera (its top three rows are read: R = the 3x3
 * block, t = the last column) are DEVICE pointers: the pose comes straight from the chain of sde_pose_compose.  C is taken as rigid, camera ->
 * world being R^T (p - t): that is the CALLER's responsibility, a C that is not rigid renders a sheared volume.  Destinations:
 *   depth   [H,W]   fp32: the z-depth of the surface, 0 where the ray finds none (a miss);
 *   normal  [H,W,3] fp32, or NULL (not wanted): the unit normal in camera coordinates, towards positive tsdf; 0, 0, 0 on a miss;
 *   picture [H,W,4] uint8, 4-byte aligned, or NULL; refused with rgba == NULL: the voxel colour with alpha 255; 0, 0, 0, 0 on a miss.
 * near, step (fp32) and the sample count n are host arguments.  For the pixel (u, v), in fp32 in exactly this order, nothing fused, every division
 * and the square root correctly rounded:
 *   0. with k00 = 1 / fx, k02 = (-1 * cx) / fx, k11 = 1 / fy, k12 = (-1 * cy) / fy:  rx = k00 * (float)u + k02;  ry = k11 * (float)v + k12;  the ray
 *      is (rx, ry, 1).  If one of the twelve entries of C that are read or one of fx, cx, fy, cy is not finite, EVERY pixel is a miss.
 *   1. sample i = 0 .. n-1 lies at the z-depth s_i = near + (float)i * step (from i, never accumulated);   p = (s * rx, s * ry, s);
 *      d_k = p_k - t_k;   w_r = (R_0r * d_0 + R_1r * d_1) + R_2r * d_2   for r = x, y, z;   g_r = (w_r - origin_r) / voxel - 0.5f;
 *      b_r = floorf(g_r);   f_r = g_r - b_r.
 *   2. the sample is VALID iff every g_r is finite (compared first: no integer conversion is undefined), 0 <= b_r <= n_r - 2 on every axis and all
 *      eight voxels (bx + dx, by + dy, bz + dz), dx, dy, dz in {0, 1}, have weight >= min_weight.  With T_zyx their tsdf:
 *   3. c_zy = T_zy0 + fx * (T_zy1 - T_zy0);   e_z = c_z0 + fy * (c_z1 - c_z0);   the sample's value t = e_0 + fz * (e_1 - e_0).
 *   4. the march: a valid sample becomes prev, an invalid one clears prev.  The FIRST i with prev set, t_prev > 0 and t_i <= 0 is the hit; a
 *      crossing from negative to positive is none and the march goes on; no hit in n samples is a miss.
 *      depth = s_{i-1} + step * (t_prev / (t_prev - t_i)),   s_{i-1} = near + (float)(i - 1) * step.
 *   5. normal and colour come from sample i's cell (valid by construction), up to one step behind the surface: the gradient of the interpolant at f,
 *      X_zy = T_zy1 - T_zy0;   x_z = X_z0 + fy * (X_z1 - X_z0);   gx = x_0 + fz * (x_1 - x_0);
 *      y_z = c_z1 - c_z0;      gy = y_0 + fz * (y_1 - y_0);       gz = e_1 - e_0;
 *      m_r = (R_r0 * gx + R_r1 * gy) + R_r2 * gz;   len = sqrtf((gx * gx + gy * gy) + gz * gz);   normal_r = m_r / len, or 0, 0, 0 when len is 0
 *      or not finite.  colour: rgba of the voxel (bx + (fx >= 0.5f), by + (fy >= 0.5f), bz + (fz >= 0.5f)), alpha replaced by 255.
 * The result is that of the full march.  Because an invalid sample only clears prev and s_i does not depend on history, the kernel skips runs of
 * samples it has PROVED invalid without touching memory (the ray against the box of valid grid coordinates, widened by a bound on the rounding
 * of step 1) and no others; a ray that never enters the box reads nothing of the volume.  A grid with a dimension of 1 has no cells: every pixel
 * is a miss.  One launch, one thread per pixel, no atomics, no workspace, no allocation, no host synchronisation: legal under graph capture, the
 * same bytes every run; nothing but the three destinations is written.  Refused before any launch: dims outside the limits, voxel <= 0,
 * min_weight < 1 (or a NaN), H or W outside [1, 32768], n outside [1, 65536], step <= 0, near or step not finite, NULL tsdf / weight / origin /
 * K / C / depth, a picture with rgba == NULL, rgba or picture off a 4-byte boundary. */
int sde_pose_compose(const float* T, float* C, sde_stream_t stream);
int sde_tsdf_integrate(const float* pred, int ph, int pw, const int* ymap, const int* xmap, int H, int W, const uint8_t* frame, const float* K,
                       const float* C, const float* origin, float voxel, float trunc, float max_weight, float min_depth, float max_depth,
                       float* tsdf, float* weight, uint8_t* rgba, int nx, int ny, int nz, sde_stream_t stream);
size_t sde_tsdf_points_ws_bytes(int nx, int ny, int nz);
int sde_tsdf_points(const float* tsdf, const float* weight, const uint8_t* rgba, int nx, int ny, int nz, const float* origin, float voxel,
                    float min_weight, void* workspace, size_t workspace_bytes, void* points, long cap, int* count, sde_stream_t stream);
size_t sde_tsdf_mesh_ws_bytes(int nx, int ny, int nz);
int sde_tsdf_mesh(const float* tsdf, const float* weight, const uint8_t* rgba, int nx, int ny, int nz, const float* origin, float voxel,
                  float min_weight, void* workspace, size_t workspace_bytes, void* vertices, long cap_vertices, int* faces, long cap_faces,
                  int* count, sde_stream_t stream);
int sde_tsdf_render(const float* tsdf, const float* weight, const uint8_t* rgba, int nx, int ny, int nz, const float* origin, float voxel,
                    float min_weight, const float* K, const float* C, int H, int W, float near, float step, int n, float* depth, float* normal,
                    uint8_t* picture, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Frame-to-model alignment: the camera tracked against the TSDF volume (csrc/align.hip; binding and host twins in hip/align.py).  ONE call of
 * sde_frame_align is ONE Gauss-Newton iteration of a point-to-plane fit of the current frame's depth to the model that sde_tsdf_render shows
 * from the PREDICTED pose C, together with the update of one depth scale.  No counterpart in the reference.
 *
 * state: SDE_ALIGN_STATE_WORDS (40) 4-byte words of DEVICE memory, 4-byte aligned:
 *   words  0..15  D    [4,4] fp32 row-major: the current frame's camera coordinates -> the render camera's.  World -> corrected camera is D^-1 C.
 *   words 16..31  Dinv [4,4] fp32 row-major: its rigid inverse [R^T | -R^T t].
 *   word  32      s    fp32: the scale the frame's depth is multiplied by              (SDE_ALIGN_SCALE_AT)
 *   word  33      fp32:  the last iteration's sum of r^2 over the pose inliers         (SDE_ALIGN_SUMSQ_AT)
 *   word  34      int32: the last iteration's pose-inlier count                        (SDE_ALIGN_COUNT_AT)
 *   word  35      int32: the last iteration's scale-inlier count                       (SDE_ALIGN_SCALE_COUNT_AT)
 *   word  36      int32: the last iteration's status, SDE_ALIGN_OK / _TOO_FEW / _SINGULAR  (SDE_ALIGN_STATUS_AT)
 *   words 37..39  reserved: written as 0 by the reset, never afterwards.
 * sde_frame_align_reset: D = Dinv = I, s = 1, words 33..39 all bits zero.  One launch of one workgroup.
 *
 * sde_frame_align.  pred [ph,pw], ymap [H], xmap [W], K [3,3]: the contract of sde_tsdf_integrate.  model_depth [H,W] (z-depth, 0 = miss) and
 * model_normal [H,W,3] (camera coordinates) are sde_tsdf_render's outputs.  mode: SDE_ALIGN_POSE | SDE_ALIGN_SCALE.  Two launches ordered on
 * the stream.
 *
 * ACCUMULATE.  One thread per pixel, workgroups of 256 threads on a grid of ceil(W / 32) x ceil(H / 8): thread t of workgroup (bx, by) has
 * wave = t / 64, lane = t % 64 and the pixel u = 32 bx + 8 wave + lane % 8, v = 8 by + lane / 8 (sde_tsdf_render's tile).  In fp32, in exactly
 * this order, nothing fused, every division correctly rounded; D and s are the state's on entry:
 *   1. kept iff u < W and v < H;   my = ymap[v];  mx = xmap[u];                         kept iff both >= 0;
 *      d0 = pred[my * pw + mx];                                                         kept iff d0 is finite and min_depth < d0 <= max_depth;
 *      d = s * d0;
 *   2. with k00 = 1 / fx, k02 = (-1 * cx) / fx, k11 = 1 / fy, k12 = (-1 * cy) / fy:  rx(u) = k00 * (float)u + k02;  ry(v) = k11 * (float)v + k12;
 *      p = (d * rx(u), d * ry(v), d);
 *   3. q_r = ((D_r0 * p_x + D_r1 * p_y) + D_r2 * p_z) + D_r3  for r = x, y, z;           kept iff q_z is finite and > 0;
 *   4. step 2 of sde_tsdf_integrate on q: X = (fx * q_x + cx * q_z) / (q_z + 1e-6f), Y likewise, rintf, |.| < 1e9f, 0 <= ix < W, 0 <= iy < H;
 *   5. m = model_depth[iy * W + ix];                                                    kept iff m > 0;
 *      n = model_normal[iy * W + ix];                                                   kept iff not (n_x == 0 and n_y == 0 and n_z == 0);
 *   6. g = (m * rx(ix), m * ry(iy), m);   e = q - g;   r = (n_x * e_x + n_y * e_y) + n_z * e_z;
 *   7. POSE INLIER iff |r| <= dist_tol * m (a NaN is none).  With c = (q_y n_z - q_z n_y, q_z n_x - q_x n_z, q_x n_y - q_y n_x) and
 *      J = (c_x, c_y, c_z, n_x, n_y, n_z) the pixel's terms are
 *        term[k] = J_i * J_j for i <= j, k = 0..20 in the order (0,0), (0,1), .. (0,5), (1,1), .. (5,5);   term[21 + i] = J_i * r;
 *        term[27] = r * r;   term[28] = 1;
 *   8. rho = m / q_z;   SCALE INLIER iff |rho - 1| <= scale_tol:   term[29] = rho;   term[30] = 1.   Step 8 does not depend on step 7.
 *   Every term that is not set, term[31] and all terms of a pixel that is not kept are 0.
 * The workgroup's 32 sums, each in this order: the 64 terms of a wave as a balanced binary tree over the lanes ((l0 + l1) + (l2 + l3)) + ...;
 * then the four waves ((w0 + w1) + w2) + w3.  Row by * gridDim.x + bx of the slab [rows][32] in the workspace receives them.  Every workgroup
 * writes its whole row: the workspace's contents on entry do not matter.
 *
 * FINISH, fp64 from here on until the stores.  Column k of the slab: S_g = the rows g, g + 32, g + 64, ... added in ascending order starting
 * from 0.0, for g = 0..31; then the 32 S_g as a balanced binary tree (S_0 + S_1) + (S_2 + S_3) ...  The totals of columns 28 and 30 are the
 * counts (exact).  Words 33, 34, 35 are written every time (word 33 = the total of column 27 rounded to fp32).  Then, in this order:
 *   1. count < min_count: status SDE_ALIGN_TOO_FEW, nothing else is written.
 *   2. with SDE_ALIGN_POSE: A = the symmetric 6 x 6 matrix of the totals 0..20, b_i = total[21 + i];  A_ii = A_ii * (1.0 + (double)damping).
 *      LDL^T without pivoting, for j = 0..5:  d_j = A_jj - sum_{c<j} (L_jc * L_jc) * d_c;  for i > j:  L_ij = (A_ij - sum_{c<j} (L_ic * L_jc) * d_c) / d_j;
 *      every sum subtracted term by term for ascending c.  y_i = -b_i - sum_{c<i} L_ic * y_c (ascending i);  z_i = y_i / d_i;
 *      xi_i = z_i - sum_{c>i} L_ci * xi_c (descending i, ascending c).  A pivot d_j that is <= 0 or not finite, or a (float)xi_i that is not
 *      finite: status SDE_ALIGN_SINGULAR, nothing else is written.
 *   3. xi = (omega, v).  a = 0.5 * omega;  aa = (a_0 * a_0 + a_1 * a_1) + a_2 * a_2;  the Cayley rotation, each entry rounded to fp32 once:
 *        R_ii = ((1.0 - aa) + 2.0 * (a_i * a_i)) / (1.0 + aa);     R_ij = (2.0 * (a_i * a_j) + 2.0 * x_ij) / (1.0 + aa)  with  x_01 = -a_2, x_02 = a_1,
 *        x_10 = a_2, x_12 = -a_0, x_20 = -a_1, x_21 = a_0 (the second product is exact; a_i * a_j with the smaller index first).  T = [R | (float)v].
 *   4. D <- T * D in fp32 in sde_pose_compose's order; Dinv_rc = D_cr, Dinv_r3 = -((D_0r * D_03 + D_1r * D_13) + D_2r * D_23) of the new D; the
 *      bottom rows are not touched.
 *   5. with SDE_ALIGN_SCALE and scale count >= min_count:  s <- s * (float)(total[29] / (double)scale count)   (one fp32 product).
 *   6. status SDE_ALIGN_OK.
 * Both launches: no atomics, no ticket, no workgroup waits for another, no allocation, no host synchronisation: legal under graph capture, the
 * same bytes every run; nothing is written but the state and the workspace.  workspace: sde_frame_align_ws_bytes(H, W) bytes (0 for sizes the
 * entry point refuses), 4-byte aligned.  Refused before any launch: H or W outside [1, 32768], ph or pw <= 0, a NULL pointer, a state off a
 * 4-byte boundary, mode outside 1..3, dist_tol or scale_tol <= 0 (or a NaN), damping < 0 (or a NaN), min_count < 6, min_depth >= max_depth (or
 * a NaN), a workspace that is NULL, misaligned or too small. */
#define SDE_ALIGN_POSE 1
#define SDE_ALIGN_SCALE 2
#define SDE_ALIGN_OK 0
#define SDE_ALIGN_TOO_FEW 1
#define SDE_ALIGN_SINGULAR 2
#define SDE_ALIGN_SUMS 32
#define SDE_ALIGN_STATE_WORDS 40
#define SDE_ALIGN_SCALE_AT 32
#define SDE_ALIGN_SUMSQ_AT 33
#define SDE_ALIGN_COUNT_AT 34
#define SDE_ALIGN_SCALE_COUNT_AT 35
#define SDE_ALIGN_STATUS_AT 36
size_t sde_frame_align_ws_bytes(int H, int W);
int sde_frame_align_reset(float* state, sde_stream_t stream);
int sde_frame_align(const float* pred, int ph, int pw, const int* ymap, const int* xmap, int H, int W, const float* K, const float* model_depth,
                    const float* model_normal, float min_depth, float max_depth, float dist_tol, float scale_tol, int min_count, float damping,
                    int mode, float* state, void* workspace, size_t workspace_bytes, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * MotionLearning loss stack (csrc/motion_loss.hip; autograd wrappers in hip/motion_loss.py).  fp32, planar NCHW, no host synchronisation.
 *
 * sde_view_synthesis_pp: detectron2/geometry/camera.py:L166-202 with a per-pixel translation t [B,3,H,W] and a 3x3 rotation R [B,3,3]; the
 * outputs of sde_view_synthesis (Z, grid, valid optional).  The projection keeps that entry point's fp32 operation order; K @ t is formed per pixel.
 *
 * sde_rgbd_fwd / sde_rgbd_bwd: detectron2/modeling/meta_arch/MotionLearning.py:L248-291 for N samples (both directions of a pair stack along N).
 * frame_* [N,3,H,W], depth_* [N,1,H,W], K, R [N,3,3], t [N,3,H,W]; ssim != 0 adds the WeightedSSIM term (C1 or C2 may be +inf: that factor is
 * dropped, ssim_loss.py:L99-104).  Forward, three launches: sampled [N,3,H,W] (warped frame_B), grid [N,H,W,2] (coords_A_in_B), occ [N,1,H,W]
 * (occlusion mask), err [N,1,H,W] (depth_in_B - sampled depth_B), valid [N,1,H,W] (projection mask), dpw [N,1,H,W] (depth_proximity_weight),
 * part1 [sde_rgbd_num_blocks][4] and part2 [sde_rgbd_num_blocks] workspaces, stats [4][N] = per-sample sum |sampled - frame_A| occ,
 * sum ssim_map avg_w, sum |err| occ / normalizer, normalizer.  Backward, three launches: g_l1 / g_ssim / g_dl1 [N] are the upstream gradients
 * of stats rows 0 / 1 / 2 (NULL: zero; the SSIM row's is multiplied by gscale_ssim), coef [N,3,H,W,4] workspace (16-byte aligned),
 * d_depth [N,1,H,W], d_t [N,3,H,W], dR_partial [sde_rgbd_num_blocks][9] workspace, dR [N,3,3].  frame_*, K and depth_B receive no gradient.
 *
 * sde_wssim_fwd / sde_wssim_bwd: ssim_loss.py:L56-111, (x, y [N,C,H,W], w [N,1,H,W]) -> (map [N,C,H,W], avg_w [N,1,H,W]); gradients of the map
 * to x and y (either may be NULL), coef [N,C,H,W,4] workspace.
 *
 * sde_motion_consistency_fwd / _bwd: detectron2/modeling/losses/motion_loss.py:L7-48.  grid [N,H,W,2] (a constant), mask [N,1,H,W], R_* [N,3,3],
 * t_* [N,3,H,W]; out[2] = rot_error, trans_error; partial [sde_rgbd_num_blocks] workspace.  Backward: g_rot / g_trans device scalars (NULL: zero),
 * d_tB_zeroed [N,3,H,W] must be zero on entry (the bilinear taps are scattered into it with fp32 atomic adds: the one sum of this stack whose
 * order is not fixed), dR_partial [sde_rgbd_num_blocks][9] workspace.
 *
 * sde_motion_smooth_* / sde_motion_sparsity_*: motion_loss.py:L51-64 over planes = B * C maps; one launch each way.  partial: workspace of
 * sde_motion_smooth_num_blocks / planes floats; ticket: one device int, zero between launches; mean [planes]: the per-plane mean |f| (kept for
 * the backward).  out / gout: device scalars.
 *
 * sde_avgpool_fwd / _bwd: F.adaptive_avg_pool2d (camera.py:L49-54), [planes,H,W] <-> [planes,h,w]. */
typedef struct sde_rgbd_desc {
    const float *frame_A, *frame_B, *depth_A, *depth_B, *K, *R, *t;
    int32_t N, H, W, ssim;
    float C1, C2;
} sde_rgbd_desc;
int sde_view_synthesis_pp(const float* img, const float* depth, const float* K, const float* R, const float* t, int B, int C, int H, int W, float* sampled,
                          float* Z, float* grid, uint8_t* valid, sde_stream_t stream);
int sde_rgbd_num_blocks(int N, int H, int W);
int sde_rgbd_fwd(const sde_rgbd_desc* d, float* sampled, float* grid, float* occ, float* err, uint8_t* valid, float* dpw, float* part1, float* part2,
                 float* stats, sde_stream_t stream);
int sde_rgbd_bwd(const sde_rgbd_desc* d, const float* sampled, const float* occ, const float* err, const float* dpw, const float* stats, const float* g_l1,
                 const float* g_ssim, const float* g_dl1, float gscale_ssim, float* coef, float* d_depth, float* d_t, float* dR_partial, float* dR,
                 sde_stream_t stream);
int sde_wssim_fwd(const float* x, const float* y, const float* w, int N, int C, int H, int W, float C1, float C2, float* map, float* avg_w, sde_stream_t stream);
int sde_wssim_bwd(const float* x, const float* y, const float* w, const float* gout, int N, int C, int H, int W, float C1, float C2, float* coef, float* dx,
                  float* dy, sde_stream_t stream);
int sde_motion_consistency_fwd(const float* grid, const float* mask, const float* R_A2B, const float* R_B2A, const float* t_A2B, const float* t_B2A, int N, int H,
                               int W, float* partial, float* out, sde_stream_t stream);
int sde_motion_consistency_bwd(const float* grid, const float* mask, const float* R_A2B, const float* R_B2A, const float* t_A2B, const float* t_B2A,
                               const float* g_rot, const float* g_trans, int N, int H, int W, float* d_tA, float* d_tB_zeroed, float* dR_partial, float* dR_A2B,
                               float* dR_B2A, sde_stream_t stream);
int sde_motion_smooth_num_blocks(int planes, int H, int W);
int sde_motion_smooth_fwd(const float* f, int planes, int H, int W, float* partial, float* out, int* ticket, sde_stream_t stream);
int sde_motion_smooth_bwd(const float* f, const float* gout, int planes, int H, int W, float* df, sde_stream_t stream);
int sde_motion_sparsity_fwd(const float* f, int planes, long hw, float* mean, float* partial, float* out, int* ticket, sde_stream_t stream);
int sde_motion_sparsity_bwd(const float* f, const float* mean, const float* gout, int planes, long hw, float* df, sde_stream_t stream);
int sde_avgpool_fwd(const float* src, float* dst, int planes, int H, int W, int h, int w, sde_stream_t stream);
int sde_avgpool_bwd(const float* dout, float* din, int planes, int H, int W, int h, int w, sde_stream_t stream);

/* Per-scale glue of MotionLearningModel (MotionLearning.py:L126-166, L205-208), both directions stacked along the batch: N = 2B, samples [0, B) are
 * frame 1 -> 2 and [B, 2B) frame 2 -> 1.  fp32 planar NCHW, no host synchronisation, no float atomics (forward and backward repeat bit for bit).
 *
 * sde_motion_prep_fwd: depth [N,1,H0,W0], motion [N,3,H0,W0] or null, t_pose [N,3], mask01 [N,1,H0,W0] or null (0/1, already dilated), target (h, w):
 *   depth_r = adaptive_avg_pool(depth); m_r = adaptive_avg_pool(motion * mask01); t = t_pose + m_r (t_pose expanded without motion);
 *   normalize: depth_mean = mean of depth_r over all N samples; depth_n = depth_r / depth_mean, t /= depth_mean, m_r /= depth_mean;
 *   m_norm = m_r / sqrt(3 mean_{c,h,w}(t^2) + 1e-12) per sample.
 *   Outputs: depth_r [N,1,h,w], depth_n (normalize only; depth_r otherwise), t [N,3,h,w], overall [N,3,h,w] = t before the division (normalize only; t
 *   otherwise), m_norm [N,3,h,w] (with motion), and optionally depth_n_sw / t_sw: depth_n and t with the two halves of the batch exchanged.
 *   Workspaces: partial [sde_rgbd_num_blocks(N,h,w)][2], stats [2 + 4N] (kept for the backward), ticket: one device int, zero between launches
 *   (the kernels leave it at zero).
 * sde_motion_prep_bwd: gradients of depth_r, depth_n, t, t_sw and m_norm (each may be null = zero) -> d_depth [N,1,H0,W0], d_motion [N,3,H0,W0] (times
 *   mask01; null without motion), d_tpose [N,3].  The gradient flows through depth_mean and through the per-sample mean of t^2.
 *   Workspaces: partial [sde_rgbd_num_blocks(N,h,w)][9], bstats [1 + 10N], ticket as above.
 * sde_mask_dilate: max_pool2d(mask > 0, 2d + 1, stride 1, padding d) of [planes,H,W] as a 0/1 float map, separable; d >= 1 may exceed the image; tmp: a
 *   second [planes,H,W] buffer. */
int sde_motion_prep_fwd(const float* depth, const float* motion, const float* t_pose, const float* mask01, int N, int H0, int W0, int h, int w, int normalize,
                        float* depth_r, float* depth_n, float* t, float* overall, float* m_norm, float* depth_n_sw, float* t_sw, float* partial, float* stats,
                        int* ticket, sde_stream_t stream);
int sde_motion_prep_bwd(const float* mask01, const float* depth_n, const float* t, const float* m_norm, const float* stats, const float* g_depth_r,
                        const float* g_depth_n, const float* g_t, const float* g_t_sw, const float* g_m_norm, int N, int H0, int W0, int h, int w, int normalize,
                        float* partial, float* bstats, int* ticket, float* d_depth, float* d_motion, float* d_tpose, sde_stream_t stream);
int sde_mask_dilate(const float* mask, float* tmp, float* out, int planes, int H, int W, int d, sde_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * DenseNet dense blocks without the concatenation (csrc/dense.hip; autograd wrappers in hip/dense.py): torchvision's _DenseLayer computes
 * relu(norm1(torch.cat(features, 1))) over a map that grows by `growth_rate` channels per layer.  Here the block stays in PIECES -- the block input
 * [M,C0] and one [M,g] tensor per layer, each NHWC-contiguous, the plain output of that layer's 3x3 convolution -- named by a descriptor that is
 * passed to the kernels by value (no upload; legal under graph capture).  fp32 and bf16, every piece width a multiple of 8; anything else (fp16
 * included) is refused before a launch.  Nothing allocates or synchronises, workspace sizes depend on shape only, no floating-point atomics: two
 * runs give the same bits.
 *
 * sde_dense_stats: the (sum, sum of squares) slab [rows(+SDE_REDUCE_ROWS, unused)][C][2] the producing convolution wrote for a NEW piece (or
 *   sde_channel_stats for the block input) -> rows [off, off + C) of the block's table [Ct][2] = (mean, biased variance) over `count` pixels.
 *   One launch per piece; later layers only read the table.
 * sde_dense_bn_relu_fwd: out [M,Cin] = relu(batch_norm(cat(pieces))), Cin = sum of the piece widths, the contiguous operand of the 1x1
 *   convolution that follows.  table != NULL (training): batch statistics from the table's first Cin rows; running_mean / running_var (optional,
 *   both or neither) are updated with `momentum` and the unbiased variance, as torch does.  table == NULL (eval): the running statistics.
 *   bnp [4][Cin] (mean, rstd, scale, shift) is written for the backward pass.  Two launches (parameters, apply).
 * sde_dense_bn_relu_bwd: g [M,Cin] = gradient of `out`; the pieces are gathered again and the ReLU mask re-derived.  part: workspace
 *   [sde_dense_bwd_rows(M, Cin, dtype)][Cin][2].  dx [M,Cin] (one contiguous tensor); dgamma / dbeta [Cin] (either may be NULL: frozen
 *   parameters), (+)= when accumulate_params.  Two launches (reduce, apply).
 * sde_dense_bwd_rows: partial rows of that workspace; shape-only (negative: unsupported dtype or width).
 * sde_dense_grad_gather: out [M,g] = [outside [M,g] +] sum over the descriptor's n tensors dx_k [M, C[k]] of their columns [off, off + g), in
 *   that order with fp32 accumulation: the gradient of the piece that sits at channel offset `off` of its n later consumers.
 * sde_avgpool2x2_fwd / _bwd: nn.AvgPool2d(2, 2) of a transition, x [B,H,W,C] <-> out [B,H/2,W/2,C] (odd sizes floor; the odd last row / column
 *   receives a zero gradient). */
#define SDE_DENSE_MAX 40
typedef struct sde_dense_desc {
    const void* p[SDE_DENSE_MAX];
    int32_t C[SDE_DENSE_MAX]; /* piece widths (sde_dense_grad_gather: row widths of the dx tensors) */
    int32_t n, reserved;
} sde_dense_desc;
int sde_dense_stats(const float* slab, int rows, int C, long count, float* table, int off, sde_stream_t stream);
int sde_dense_bwd_rows(long M, int Cin, int dtype);
int sde_dense_bn_relu_fwd(const sde_dense_desc* d, long M, int dtype, const float* table, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, float* bnp, void* out, sde_stream_t stream);
int sde_dense_bn_relu_bwd(const sde_dense_desc* d, long M, int dtype, const void* g, const float* bnp, float* part, float* dgamma, float* dbeta,
                          int accumulate_params, void* dx, sde_stream_t stream);
int sde_dense_grad_gather(const sde_dense_desc* dxs, long M, int off, int g, int dtype, const void* outside, void* out, sde_stream_t stream);
int sde_avgpool2x2_fwd(const void* x, int B, int H, int W, int C, int dtype, void* out, sde_stream_t stream);
int sde_avgpool2x2_bwd(const void* dout, int B, int H, int W, int C, int dtype, void* dx, sde_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SDE_HIP_H */
