"""Run a trained depth model on an image or a folder of frames (the reference's tools/demo.py on the HIP path):

    python -m simpledepthestimation_amd.tools.demo --cfg output/run/config.yaml --input frames/ --output imgs/ --opts MODEL.WEIGHTS output/run/model_final.pth

For every input file `<output>/<stem>.png` is the stacked picture of demo.py:L100-104: the camera frame on top, the depth map below it in
matplotlib's `magma` colours of depth ** 0.8 over [0, MODEL.MAX_DEPTH ** 0.8].  Frames go through DepthPredictor.stream: the preprocess chain of
DATASETS.TEST.PREPROCESS (KBCrop when it names none), the model, the way back to the frame's size and the colours run on the GPU, the next
frame is uploaded and the previous picture downloaded meanwhile."""
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
    p.add_argument("--opts", default=[], nargs=argparse.REMAINDER, help="config overrides as KEY VALUE pairs, e.g. MODEL.WEIGHTS model.pth")
    return p.parse_args(argv)


def input_files(path):
    """demo.py:L52-53: the sorted entries of a directory, or the one file."""
    return [os.path.join(path, f) for f in sorted(os.listdir(path))] if os.path.isdir(path) else [path]


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
    results = predictor.stream((read_rgb(f) for f in files), frame_in_canvas=not args.no_frame, want_u16=args.save_depth)
    for path, res in zip(files, results):
        stem = os.path.splitext(os.path.basename(path))[0]
        Image.fromarray(res["canvas"]).save(os.path.join(args.output, stem + ".png"), format="PNG", compress_level=3)
        if args.save_depth:
            Image.fromarray(np.ascontiguousarray(res["depth_u16"])).save(os.path.join(args.output, stem + "_depth.png"), format="PNG", compress_level=3)
    print(f"{len(files)} picture(s) written to {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
