"""Run a trained depth model on an image or a folder of frames (the reference's tools/demo.py on the HIP path):

    python -m simpledepthestimation_amd.tools.demo --cfg output/run/config.yaml --input frames/ --output imgs/ --opts MODEL.WEIGHTS output/run/model_final.pth

For every input file `<output>/<stem>.png` is the stacked picture of demo.py:L100-104: the camera frame on top, the depth map below it in
matplotlib's `magma` colours of depth ** 0.8 over [0, MODEL.MAX_DEPTH ** 0.8].  Frames go through DepthPredictor.stream: the preprocess chain of
DATASETS.TEST.PREPROCESS (KBCrop when it names none), the model, the way back to the frame's size and the colours run on the GPU, the next
frame is uploaded and the previous picture downloaded meanwhile.

With --save-cloud --intrinsics fx fy cx cy, `<stem>.ply` holds the frame's coloured point cloud: every pixel (every --cloud-step-th in both
directions) whose depth lies in (MODEL.MIN_DEPTH where the config has one, else 0; MODEL.MAX_DEPTH], lifted through the given intrinsics of the
input frames, in raster order.  The file is a binary_little_endian PLY whose vertex is the 16-byte record of sde_depth_cloud."""
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
    p.add_argument("--cloud-step", type=int, default=1, help="the cloud takes every N-th pixel of every N-th row (default 1: all)")
    p.add_argument("--opts", default=[], nargs=argparse.REMAINDER, help="config overrides as KEY VALUE pairs, e.g. MODEL.WEIGHTS model.pth")
    args = p.parse_args(argv)
    if args.save_cloud and args.intrinsics is None:
        p.error("--save-cloud needs --intrinsics fx fy cx cy")
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
