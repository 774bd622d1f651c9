"""The triangle mesh of a TSDF volume (TsdfVolume.mesh, sde_tsdf_mesh: four launches) against the surface points of the same volume
(TsdfVolume.points, sde_tsdf_points: three launches), on the volume the launch part of scripts/bench_volume.py builds: --dims voxels of
vmax / dims_z, one uniform random prediction over [2, vmax] integrated from the middle of the near face (MonoDepth2's plan of a 375 x 1242 frame).

    points_us / mesh_us   GPU time of one call, from a graph of --reps calls replayed --replays times between two events.  The two are timed in
                          alternating rounds (points, mesh, points, mesh, ...) in two runs of --rounds rounds each: per run the median and
                          spread_pct, the largest (max - min) / median of either call's rounds.  points_first_us / points_last_us are the
                          medians of the first and of the last run's points rounds: the yardstick before and after, in one session
    mesh_vertices / mesh_triangles / points_found   what the calls count
    mesh_bytes            what each launch has to move, counted from the shapes and the counts: `count` 8 B per voxel (weight and tsdf; the
                          other seven corners of a cell are neighbours' voxels: cache) + 8 B per tile written; `scan` 16 B per tile;
                          `vertices` 8 B per voxel + 4 B per tile + per vertex 16 B record, 4 B map and the 32 B of its cell's eight corner colours; `faces` 8 B per voxel +
                          4 B per tile + per quad 16 B of map and 24 B of indices.  The second and third read of the grid come from a
                          256 MiB last-level cache that holds the 64 MiB of tsdf and weight: the sum over the time is NOT a share of HBM bandwidth.

    python scripts/bench_mesh.py [--reps 50] [--replays 10] [--rounds 5] [--dims 256 256 128] [--out profiles/mesh_bench.txt]

Prints one JSON line and appends it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pairs import H, KITTI_K, W, make_cfg  # noqa: E402


def build_volume(dims, dtype, dev):
    """The volume of bench_volume.py's launch part, after one integrate."""
    from simpledepthestimation_amd.engine.predictor import PairPredictor
    from simpledepthestimation_amd.hip.present import device_maps
    from simpledepthestimation_amd.hip.volume import TsdfVolume
    from simpledepthestimation_amd.modeling import build_model
    cfg = make_cfg("MonoDepth2", dtype, dev)
    torch.manual_seed(0)
    pair_p = PairPredictor(cfg, model=build_model(cfg).eval(), use_graph=False)
    vmax = float(cfg.MODEL.MAX_DEPTH)
    plan = pair_p.plan(H, W)
    ymap, xmap = device_maps(*plan.maps((plan.h, plan.w)), plan.h, plan.w, dev)
    fr = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    pred = torch.rand(1, plan.h, plan.w, device=dev) * (vmax - 2) + 2
    vol = TsdfVolume(dims, vmax / dims[2], min_depth=0.0, max_depth=vmax, device=dev)
    vol.integrate(pred, ymap, xmap, torch.from_numpy(KITTI_K).to(dev), torch.eye(4, device=dev), frame=fr)
    return vol


def bench(args, dev):
    vol = build_volume(tuple(args.dims), args.dtype, dev)
    voxels = int(vol.weight.numel())
    points, pcount = vol.points()
    pws = torch.empty(vol.workspace_numel(), dtype=torch.int32, device=dev)
    vertices, faces, mcount = vol.mesh()
    mws = torch.empty(vol.mesh_workspace_numel(), dtype=torch.int32, device=dev)
    calls = {"points": lambda: vol.points(out=(points, pcount), workspace=pws), "mesh": lambda: vol.mesh(out=(vertices, faces, mcount), workspace=mws)}
    graphs = {}
    for name, call in calls.items():
        call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.reps):
                call()
        g.replay()
        graphs[name] = g

    def us(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.replays):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3 / (args.reps * args.replays), 2)

    runs = []
    for _ in range(2):
        rounds = {"points": [], "mesh": []}
        for _ in range(args.rounds):                                     # alternating: the two calls see the same neighbours
            for name in ("points", "mesh"):
                rounds[name].append(us(graphs[name]))
        med = {k: float(np.median(v)) for k, v in rounds.items()}
        runs.append({"points_us": rounds["points"], "mesh_us": rounds["mesh"], "points_median_us": med["points"], "mesh_median_us": med["mesh"],
                     "spread_pct": round(100 * max((max(v) - min(v)) / med[k] for k, v in rounds.items()), 2)})
    nv, nf, found = int(mcount[0].item()), int(mcount[1].item()), int(pcount.item())
    assert nv <= vertices.shape[0] and nf <= faces.shape[0], "the default caps cut the mesh: the scatter passes were not timed in full"
    tiles, quads = pws.numel(), nf // 2
    launches = {"count": 8 * voxels + 8 * tiles, "scan": 16 * tiles, "vertices": 8 * voxels + 4 * tiles + 52 * nv,
                "faces": 8 * voxels + 4 * tiles + 40 * quads}
    return {"bench": "mesh", "dims": list(args.dims), "voxels": voxels, "reps": args.reps, "replays": args.replays, "runs": runs,
            "points_first_us": runs[0]["points_median_us"], "points_last_us": runs[1]["points_median_us"],
            "mesh_over_points": [round(r["mesh_median_us"] / r["points_median_us"], 3) for r in runs],
            "points_found": found, "points_cap": int(points.shape[0]), "mesh_vertices": nv, "mesh_triangles": nf,
            "mesh_caps": [int(vertices.shape[0]), int(faces.shape[0])], "mesh_bytes": launches, "mesh_bytes_total": sum(launches.values()),
            "points_bytes": 2 * 8 * voxels + 3 * 4 * tiles + 16 * min(found, int(points.shape[0])), "workspace_bytes": [4 * pws.numel(), 4 * mws.numel()]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--dims", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh.py measures on the GPU; there is no CPU fallback"
    line = json.dumps(bench(args, "cuda:0"))
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
