"""Run a trained depth model on an image or a folder of frames (the reference's tools/demo.py on the HIP path):

    python -m simpledepthestimation_amd.tools.demo --cfg output/run/config.yaml --input frames/ --output imgs/ --opts MODEL.WEIGHTS output/run/model_final.pth

For every input file `<output>/<stem>.png` is the stacked picture of demo.py:L100-104: the camera frame on top, the depth map below it in
matplotlib's `magma` colours of depth ** 0.8 over [0, MODEL.MAX_DEPTH ** 0.8].  Frames go through DepthPredictor.stream: the preprocess chain of
DATASETS.TEST.PREPROCESS (KBCrop when it names none), the model, the way back to the frame's size and the colours run on the GPU, the next
frame is uploaded and the previous picture downloaded meanwhile.

With --save-cloud --intrinsics fx fy cx cy, `<stem>.ply` holds the frame's coloured point cloud: every pixel (every --cloud-step-th in both
directions) whose depth lies in (MODEL.MIN_DEPTH where the config has one, else 0; MODEL.MAX_DEPTH], lifted through the given intrinsics of the
input frames, in raster order.  The file is a binary_little_endian PLY whose vertex is the 16-byte record of sde_depth_cloud.

With --pairs --intrinsics fx fy cx cy the input is a sequence and the model one with a pose network (MonoDepth2, MotionLearning): frames go through
PairPredictor.stream, and every frame that has all its context frames gets its `<stem>.png` as above (and, with --save-depth / --save-cloud, its `<stem>_depth.png` /
`<stem>.ply`).  --save-flow adds `<stem>_flow.png`, the
optical flow from that frame to the next one (the previous one for a model that only looks back) on the Middlebury colour wheel, white where
nothing moves and black where the flow is undefined, and `<stem>.flo`, the same flow as a Middlebury .flo file in pixels; --rigid-only leaves the
per-pixel motion field of a GoogleMotionNet out of it.  --save-trajectory writes `trajectory.txt`, the camera-to-world pose of the frames in the
KITTI odometry format (12 numbers per line), frame by frame from the first one on -- every STRIDE-th frame when the model was trained with a
STRIDE above 1 --, up to the scale of the monocular depth.

--stabilise (with --pairs) makes the sequence's depth consistent over time: PairPredictor.stream(..., temporal=dict(alpha, tol)) warps the fused
depth of the previous frame into the current camera with the pose the model estimated and blends it with the current prediction where the two
agree within --stabilise-tol (relative; default 0.05), with weight --stabilise-alpha (default 0.5) for the warped depth.  The pictures then show
the fused depth.  --save-state adds `<stem>_state.png`, the class of every pixel at the network's size in four fixed colours: dark grey where
the pixel is new (nothing was warped there), green where the two depths were fused, orange / blue where the warped surface lies nearer / farther
than the prediction, which is then kept.  The model needs a context one frame away.

--volume NX NY NZ --voxel V (with --pairs) fuses the whole sequence into one model of the scene: PairPredictor.stream(..., volume=TsdfVolume(...))
averages every frame's depth (the fused one with --stabilise), in the range --save-cloud uses, into a truncated-signed-distance grid of NX x NY x
NZ voxels of edge V through the camera pose chained from the model's own steps, and after the last frame `volume.ply` holds the grid's zero
crossings as coloured points (the record and the PLY layout of --save-cloud), in the first frame's camera coordinates.  --volume-origin X Y Z is
the corner of the first voxel (default: the first camera at the middle of the near face), --trunc M the truncation distance (default 4 V),
--min-weight N the number of observations a voxel needs (default 1).  --save-mesh adds `volume_mesh.ply`, the same surface as a triangle mesh
(TsdfVolume.save_mesh: one vertex per grid cell the surface passes through, two triangles per crossing, coloured like the points).  All lengths are in the model's depth units: a monocular model's scale is
not aligned.  The model needs a context one frame away.

--track-volume (with --volume) tracks the camera against the model: before a frame's depth goes in, the volume is rendered from the pose the
chain predicts and the depth is aligned with it (PairPredictor.stream(..., track=...): TsdfVolume.track, sde_frame_align), which corrects the pose
and fits one depth scale per frame (--no-track-scale: the pose alone).  `trajectory.txt` (--save-trajectory) then holds the CORRECTED
camera-to-world poses, one line per target frame, the first target being the world.

--render-volume (with --volume) looks at the model while it grows: after every frame's depth has gone in, the volume is rendered from that
frame's own camera (PairPredictor.stream(..., render=...): ray casting on the device, TsdfVolume.render) and `<stem>_model.png` holds the colour
picture, `<stem>_model_depth.png` the model's depth along every pixel's ray in the --save-depth format (0 where the ray finds no surface);
--save-normals adds `<stem>_model_normal.png`, the surface normal in camera coordinates as (n * 0.5 + 0.5) * 255.  --min-weight applies."""
import argparse
import os
import sys


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m simpledepthestimation_amd.tools.demo",
                                description="Depth maps and stacked frame / depth pictures for an image or a folder of frames. "
                                            "Writes one PNG per input; there is no video file (the reference encodes one with cv2, which this package does not use).")
    p.add_argument("--cfg", required=True, help="YAML config of the run (the config.yaml the trainer wrote)")
    p.add_argument("--input", required=True, help="an image file, or a directory whose files are taken in sorted order")
    p.add_argument("--output", default="./imgs", help="directory for <stem>.png (created when missing)")
    p.add_argument("--save-depth", action="store_true", help="also write <stem>_depth.png: 16-bit PNG of depth * 255, the format of the evaluators' depth saver")
    p.add_argument("--no-frame", action="store_true", help="pictures hold the coloured depth only, without the camera frame on top")
    p.add_argument("--save-cloud", action="store_true", help="also write <stem>.ply: the coloured point cloud of the frame (needs --intrinsics)")
    p.add_argument("--intrinsics", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"), help="pinhole intrinsics of the input frames, in pixels")
    p.add_argument("--pairs", action="store_true", help="treat --input as a sequence: depth, camera motion and optical flow from a model with a pose network "
                                                        "(needs --intrinsics)")
    p.add_argument("--save-flow", action="store_true", help="with --pairs: also write <stem>_flow.png, the flow to the next frame in colours, and <stem>.flo")
    p.add_argument("--save-trajectory", action="store_true", help="with --pairs: also write trajectory.txt, the camera poses in the KITTI odometry format")
    p.add_argument("--rigid-only", action="store_true", help="with --pairs: the flow of the camera motion alone, without the per-pixel motion field")
    p.add_argument("--stabilise", action="store_true", help="with --pairs: temporally fused depth (the previous frame's depth warped by the estimated pose and "
                                                            "blended with the prediction)")
    p.add_argument("--stabilise-alpha", type=float, default=0.5, help="with --stabilise: weight of the warped depth in the blend, in [0, 1) (default 0.5)")
    p.add_argument("--stabilise-tol", type=float, default=0.05, help="with --stabilise: relative depth difference up to which the two are blended (default 0.05)")
    p.add_argument("--save-state", action="store_true", help="with --stabilise: also write <stem>_state.png, the class of every pixel in four colours")
    p.add_argument("--volume", type=int, nargs=3, metavar=("NX", "NY", "NZ"), help="with --pairs: fuse the sequence into a TSDF volume of that many voxels and "
                                                                                   "write volume.ply, its surface points (needs --voxel)")
    p.add_argument("--voxel", type=float, help="with --volume: edge length of a voxel, in the model's depth units")
    p.add_argument("--trunc", type=float, help="with --volume: truncation distance (default 4 voxels)")
    p.add_argument("--volume-origin", type=float, nargs=3, metavar=("X", "Y", "Z"), help="with --volume: corner of the first voxel in the first camera's "
                                                                                          "coordinates (default: the camera at the middle of the near face)")
    p.add_argument("--min-weight", type=float, default=1.0, help="with --volume: observations a voxel needs to count as surface (default 1)")
    p.add_argument("--save-mesh", action="store_true", help="with --volume: also write volume_mesh.ply, the surface as a triangle mesh")
    p.add_argument("--render-volume", action="store_true", help="with --volume: also write <stem>_model.png and <stem>_model_depth.png, the volume seen "
                                                                "from the frame's camera (colour, and depth * 255 as a 16-bit PNG)")
    p.add_argument("--save-normals", action="store_true", help="with --render-volume: also write <stem>_model_normal.png, (normal * 0.5 + 0.5) * 255")
    p.add_argument("--track-volume", action="store_true", help="with --volume: align every frame with the volume before its depth goes in (frame-to-model "
                                                               "tracking); trajectory.txt then holds the corrected poses")
    p.add_argument("--no-track-scale", action="store_true", help="with --track-volume: fit the pose alone and leave the depth's scale as it is")
    p.add_argument("--cloud-step", type=int, default=1, help="the cloud takes every N-th pixel of every N-th row (default 1: all)")
    p.add_argument("--opts", default=[], nargs=argparse.REMAINDER, help="config overrides as KEY VALUE pairs, e.g. MODEL.WEIGHTS model.pth")
    args = p.parse_args(argv)
    if args.save_cloud and args.intrinsics is None:
        p.error("--save-cloud needs --intrinsics fx fy cx cy")
    if args.pairs and args.intrinsics is None:
        raise ValueError("--pairs needs --intrinsics fx fy cx cy: the flow is computed through the frames' intrinsics")
    if args.save_state and not args.stabilise:
        p.error("--save-state needs --stabilise")
    if not (0.0 <= args.stabilise_alpha < 1.0) or not args.stabilise_tol > 0.0:
        p.error("--stabilise-alpha must lie in [0, 1) and --stabilise-tol must be positive")
    if args.volume is not None:
        if args.voxel is None:
            p.error("--volume needs --voxel V")
        from ..hip.volume import check_min_weight, check_params
        try:
            check_params(args.volume, args.voxel, args.volume_origin, args.trunc)
            check_min_weight(args.min_weight)
        except ValueError as e:
            p.error(str(e))
    elif any(v is not None for v in (args.voxel, args.trunc, args.volume_origin)):
        p.error("--voxel, --trunc and --volume-origin need --volume NX NY NZ")
    elif args.save_mesh:
        p.error("--save-mesh needs --volume NX NY NZ")
    elif args.render_volume:
        p.error("--render-volume needs --volume NX NY NZ")
    elif args.track_volume:
        p.error("--track-volume needs --volume NX NY NZ")
    if args.no_track_scale and not args.track_volume:
        p.error("--no-track-scale needs --track-volume")
    if args.save_normals and not args.render_volume:
        p.error("--save-normals needs --render-volume")
    for flag in ("save_flow", "save_trajectory", "rigid_only", "stabilise", "volume"):
        if getattr(args, flag) not in (None, False) and not args.pairs:
            p.error(f"--{flag.replace('_', '-')} needs --pairs")
    if args.pairs and args.no_frame:
        p.error("--pairs does not combine with --no-frame")
    if args.cloud_step < 1:
        p.error("--cloud-step must be at least 1")
    return args


def input_files(path):
    """demo.py:L52-53: the sorted entries of a directory, or the one file."""
    return [os.path.join(path, f) for f in sorted(os.listdir(path))] if os.path.isdir(path) else [path]


PLY_PROPERTIES = (("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue"), ("uchar", "alpha"))


def ply_header(n):
    """The header of a binary little-endian PLY with n vertices laid out as hip.cloud.RECORD."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(n)}"] + [f"property {t} {name}" for t, name in PLY_PROPERTIES] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def write_ply(path, records):
    """records: the structured array of hip.cloud.as_records (x, y, z float32; red, green, blue, alpha uint8)."""
    from ..hip.cloud import RECORD
    if records.dtype != RECORD or records.ndim != 1:
        raise ValueError(f"write_ply: a 1-D array of hip.cloud.RECORD expected, got {records.dtype} {records.shape}")
    with open(path, "wb") as f:
        f.write(ply_header(records.size))
        records.tofile(f)


def trajectory_steps(results, offsets):
    """The chain of poses frame -> next frame that the records of PairPredictor.stream give, as a list of [4,4] arrays, and the position in the
    sequence of the frame the chain starts at.  A model with a context at -STRIDE supplies the step INTO its first target (the inverse of that
    target's pose to the context), so that the chain starts STRIDE frames earlier; with STRIDE above 1 every STRIDE-th record is chained."""
    from ..geometry.pose_utils import invert_pose_np
    stride = min(abs(o) for o in offsets)
    chain = [r for r in results if (r["index"] - results[0]["index"]) % stride == 0]
    steps, start = [r["pose_next"] for r in chain], chain[0]["index"]
    if stride not in offsets:                        # a model that only looks back: pose_next already is the step previous frame -> target
        return steps, start - stride
    if -stride in offsets:
        steps.insert(0, invert_pose_np(chain[0]["pose"][offsets.index(-stride)]))
        start -= stride
    return steps, start


def model_depth_u16(depth):
    """depth [H,W] float32 -> uint16 [H,W]: the fp32 product depth * 255, truncated and cut at 65535 -- the --save-depth format."""
    import numpy as np
    v = np.asarray(depth, dtype=np.float32) * np.float32(255)
    return np.where(v >= 65535, 65535, np.where(v > 0, v, 0)).astype(np.uint16)


def normal_picture(normal):
    """normal [H,W,3] float32, unit vectors or zeros -> uint8 [H,W,3]: (n * 0.5 + 0.5) * 255, truncated; a miss is mid-grey."""
    import numpy as np
    v = (np.asarray(normal, dtype=np.float32) * np.float32(0.5) + np.float32(0.5)) * np.float32(255)
    return np.clip(np.nan_to_num(v), 0, 255).astype(np.uint8)


def run_pairs(args, cfg, files):
    import numpy as np
    from PIL import Image

    from ..data.preprocess.loading import read_rgb
    from ..engine.predictor import PairPredictor
    from ..geometry.pose_utils import accumulate_poses, write_kitti_poses
    from ..hip.cloud import as_records
    from ..hip.flow import write_flo
    from ..hip.temporal import state_picture
    predictor = PairPredictor(cfg)
    fx, fy, cx, cy = args.intrinsics
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)
    j = predictor.next_context[0]                    # the context whose flow is saved: the next frame, or the previous one
    kept = []
    temporal = dict(alpha=args.stabilise_alpha, tol=args.stabilise_tol) if args.stabilise else None
    depth_range = dict(min_depth=float(cfg.MODEL.get("MIN_DEPTH", 0.0)), max_depth=float(cfg.MODEL.MAX_DEPTH))
    cloud = dict(depth_range, step=args.cloud_step) if args.save_cloud else None
    volume = None
    if args.volume is not None:
        from ..hip.volume import TsdfVolume
        volume = TsdfVolume(args.volume, args.voxel, origin=args.volume_origin, trunc=args.trunc, device=predictor.device, **depth_range)
    render = dict(normals=args.save_normals, picture=True, min_weight=args.min_weight) if args.render_volume else None
    track = dict(scale=not args.no_track_scale, min_weight=args.min_weight) if args.track_volume else None
    for res in predictor.stream((read_rgb(f) for f in files), K, rigid_only=args.rigid_only, temporal=temporal, want_u16=args.save_depth, cloud=cloud,
                                volume=volume, render=render, track=track):
        stem = os.path.splitext(os.path.basename(files[res["index"]]))[0]
        Image.fromarray(res["canvas"]).save(os.path.join(args.output, stem + ".png"), format="PNG", compress_level=3)
        if args.save_flow:
            Image.fromarray(res["flow_canvas"][j]).save(os.path.join(args.output, stem + "_flow.png"), format="PNG", compress_level=3)
            write_flo(os.path.join(args.output, stem + ".flo"), res["flow"][j])
        if args.save_depth:
            Image.fromarray(np.ascontiguousarray(res["depth_u16"])).save(os.path.join(args.output, stem + "_depth.png"), format="PNG", compress_level=3)
        if args.save_cloud:
            write_ply(os.path.join(args.output, stem + ".ply"), as_records(res["points"], res["count"])[0])
        if args.save_state:
            Image.fromarray(state_picture(res["temporal_state"])).save(os.path.join(args.output, stem + "_state.png"), format="PNG", compress_level=3)
        if render is not None:
            Image.fromarray(res["model_picture"][..., :3]).save(os.path.join(args.output, stem + "_model.png"), format="PNG", compress_level=3)
            Image.fromarray(model_depth_u16(res["model_depth"])).save(os.path.join(args.output, stem + "_model_depth.png"), format="PNG", compress_level=3)
            if args.save_normals:
                Image.fromarray(normal_picture(res["model_normal"])).save(os.path.join(args.output, stem + "_model_normal.png"), format="PNG", compress_level=3)
        kept.append({"index": res["index"], "pose": res["pose"].copy(), "pose_next": res["pose_next"]})
        if track is not None:
            kept[-1]["world_to_camera"] = res["world_to_camera"].copy()
    if not kept:
        raise SystemExit(f"--pairs: {len(files)} frame(s) are fewer than one window of the model (offsets {predictor.offsets})")
    if args.save_trajectory and track is not None:        # the corrected poses, one per target frame: the first target is the world
        from ..geometry.pose_utils import invert_pose_np
        write_kitti_poses(os.path.join(args.output, "trajectory.txt"), np.stack([invert_pose_np(r["world_to_camera"].astype(np.float64)) for r in kept]))
    elif args.save_trajectory:
        steps, _ = trajectory_steps(kept, predictor.offsets)
        write_kitti_poses(os.path.join(args.output, "trajectory.txt"), accumulate_poses(np.stack(steps)))
    if volume is not None:
        written, found = volume.save_ply(os.path.join(args.output, "volume.ply"), min_weight=args.min_weight)
        print(f"volume.ply: {written} of {found} surface point(s)")
        if args.save_mesh:
            nv, nf = volume.save_mesh(os.path.join(args.output, "volume_mesh.ply"), min_weight=args.min_weight)
            print(f"volume_mesh.ply: {nv} vertices, {nf} triangle(s)")
    print(f"{len(kept)} picture(s) written to {args.output}")
    return 0


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    from PIL import Image

    from ..config import get_cfg
    from ..data.preprocess.loading import read_rgb
    from ..engine.predictor import DepthPredictor

    cfg = get_cfg()
    cfg.set_new_allowed(True)
    cfg.merge_from_file(args.cfg)
    cfg.merge_from_list(args.opts)
    cfg.freeze()
    files = input_files(args.input)
    os.makedirs(args.output, exist_ok=True)
    if args.pairs:
        return run_pairs(args, cfg, files)
    predictor = DepthPredictor(cfg)
    extra = {}
    if args.save_cloud:
        from ..hip.cloud import as_records
        fx, fy, cx, cy = args.intrinsics
        extra = dict(intrinsics=np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32),
                     cloud=dict(min_depth=float(cfg.MODEL.get("MIN_DEPTH", 0.0)), max_depth=float(cfg.MODEL.MAX_DEPTH), step=args.cloud_step))
    results = predictor.stream((read_rgb(f) for f in files), frame_in_canvas=not args.no_frame, want_u16=args.save_depth, **extra)
    for path, res in zip(files, results):
        stem = os.path.splitext(os.path.basename(path))[0]
        Image.fromarray(res["canvas"]).save(os.path.join(args.output, stem + ".png"), format="PNG", compress_level=3)
        if args.save_depth:
            Image.fromarray(np.ascontiguousarray(res["depth_u16"])).save(os.path.join(args.output, stem + "_depth.png"), format="PNG", compress_level=3)
        if args.save_cloud:
            write_ply(os.path.join(args.output, stem + ".ply"), as_records(res["points"], res["count"])[0])
    print(f"{len(files)} picture(s) written to {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
