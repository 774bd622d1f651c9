"""Project the raw LiDAR scans of a KITTI split to the depth caches `DEPTH_TYPE: velodyne` reads:

    python -m simpledepthestimation_amd.tools.export_gt_depth --data-root kitti_raw --split splits/eigen_test.txt --cams image_02 [--out DIR]

For every split entry of a listed camera whose frame and scan exist, `<out>/<date>/<date>_drive_<drive>_sync/proj_depth/velodyne/<cam>/<id>.npz`
holds the key `velodyne_depth`: a float32 [H,W] map at the frame's size, the closest scanner point per pixel and 0 elsewhere -- the routine and
its one deviation are stated in include/sde_hip.h (sde_lidar_depth).  The scans go through the kernel in batches of frames of one size;
`--host` uses the numpy twin (hip.lidar.lidar_depth_np: the same bits) and needs no GPU.  `--out` defaults to the data root, which is where
KittiDepthV2 looks when DEPTH_ROOT equals DATA_ROOT."""
import argparse
import os
import sys

import numpy as np


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m simpledepthestimation_amd.tools.export_gt_depth",
                                description="Depth ground truth (proj_depth/velodyne/<cam>/<id>.npz) from the raw scans of a KITTI split.")
    p.add_argument("--data-root", required=True, help="the KITTI raw tree (<date>/calib_*.txt, <date>/<drive>/<cam>/data, velodyne_points/data)")
    p.add_argument("--split", required=True, help="split file: whitespace-separated <date>/<drive>/<cam>/data/<id>.png entries")
    p.add_argument("--cams", nargs="+", default=["image_02"], help="cameras to export (default image_02)")
    p.add_argument("--out", default=None, help="root of the written tree (default: --data-root)")
    p.add_argument("--vel-depth", action="store_true", help="store the scanner-frame x instead of the camera-frame z (generate_depth_map's vel_depth)")
    p.add_argument("--host", action="store_true", help="project with numpy on the host; no GPU needed")
    p.add_argument("--batch", type=int, default=16, help="scans per kernel call (default 16)")
    args = p.parse_args(argv)
    if args.batch < 1:
        p.error("--batch must be at least 1")
    return args


def out_path(root, date, drive, cam, img_id):
    return os.path.join(root, date, f"{date}_drive_{drive}_sync", "proj_depth", "velodyne", cam, f"{img_id}.npz")


def _save(path, depth):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, velodyne_depth=np.ascontiguousarray(depth, dtype=np.float32))


def _flush(group, size, vel_depth, device):
    """One kernel call for the scans of one frame size: group = [(path, scan [n,3], proj [3,4])]."""
    import torch
    from ..hip.lidar import lidar_depth
    cap = max(1, max(len(s) for _, s, _ in group))
    pts = np.zeros((len(group), cap, 3), dtype=np.float32)
    for i, (_, s, _) in enumerate(group):
        pts[i, :len(s)] = s
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    depth = lidar_depth(up(pts), up(np.array([len(s) for _, s, _ in group], dtype=np.int32)), up(np.stack([m for _, _, m in group])),
                        torch.zeros((len(group), 2), dtype=torch.int32, device=device), size[0], size[1], vel_depth=vel_depth, front_only=True).cpu().numpy()
    for (path, _, _), d in zip(group, depth):
        _save(path, d[0])


def main(argv=None):
    args = parse_args(argv)
    from PIL import Image
    from ..data.datasets.kitti_v2 import parse_split_entry, read_calib
    from ..geometry.camera import velo_to_image
    from ..hip.lidar import lidar_depth_np
    out_root = args.out or args.data_root
    device = None
    if not args.host:
        import torch
        if not torch.cuda.is_available():
            sys.exit("export_gt_depth: no GPU found; --host projects with numpy")
        device = torch.device("cuda:0")
    projs, pending, written, skipped = {}, {}, 0, 0
    for line in open(args.split, "r"):
        for entry in line.strip().split():
            date, drive, cam, img_id = parse_split_entry(entry)
            base = os.path.join(args.data_root, date, f"{date}_drive_{drive}_sync")
            img, scan_file = os.path.join(base, cam, "data", f"{img_id}.png"), os.path.join(base, "velodyne_points", "data", f"{img_id}.bin")
            if cam not in args.cams or not os.path.isfile(img) or not os.path.isfile(scan_file):
                skipped += 1
                continue
            if (date, cam) not in projs:
                projs[date, cam] = velo_to_image(read_calib(os.path.join(args.data_root, date, "calib_cam_to_cam.txt")),
                                                 read_calib(os.path.join(args.data_root, date, "calib_velo_to_cam.txt")), cam)
            with Image.open(img) as im:
                W, H = im.size
            scan = np.fromfile(scan_file, dtype=np.float32).reshape(-1, 4)[:, :3]
            path = out_path(out_root, date, drive, cam, img_id)
            if args.host:
                _save(path, lidar_depth_np(scan, projs[date, cam], (0, 0), H, W, vel_depth=args.vel_depth, front_only=True))
            else:
                group = pending.setdefault((H, W), [])
                group.append((path, scan[scan[:, 0] >= 0], projs[date, cam]))
                if len(group) >= args.batch:
                    _flush(pending.pop((H, W)), (H, W), args.vel_depth, device)
            written += 1
    for size, group in pending.items():
        _flush(group, size, args.vel_depth, device)
    print(f"export_gt_depth: {written} maps written under {out_root}, {skipped} entries skipped")
    return 0


if __name__ == "__main__":
    sys.exit(main())
