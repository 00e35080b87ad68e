"""What sub-pixel centroids cost on the bench workload (6 cameras x 1920x1080, 8 markers, 512 time steps per batch, three batches
in flight): BatchTracker with subpixel=None against subpixel={"radius": 24, "floor": 64}, in alternating runs on the same frames,
and the refine kernel's own duration from HIP events (one batch at a time, behind a blob stage, nothing else on the chip).
--baseline-only runs the subpixel=None leg alone, so that the same script also times a checkout that has no `subpixel` yet.
   python scratch/ab_subpixel.py [--steps 12] [--rounds 5] [--time-steps 512] [--baseline-only]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import Workload  # noqa: E402
from mocapv2_amd.pipeline import BatchTracker, scene_arrays  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--markers", type=int, default=8)
ap.add_argument("--steps", type=int, default=12, help="batches per timed run")
ap.add_argument("--rounds", type=int, default=5, help="alternating runs per leg")
ap.add_argument("--time-steps", type=int, default=512)
ap.add_argument("--baseline-only", action="store_true")
args = ap.parse_args()
C, W, H, T = 6, 1920, 1080, args.time_steps
SUBPIX = {"radius": 24, "floor": 64}
wl = Workload(C, W, H, args.markers, "mild")
scene = wl.scene()
K, dist, R, t, F = scene_arrays(scene)
rendered = min(32, T)
host = wl.render(scene, [(c, s) for s in range(rendered) for c in range(C)])  # 32 rendered time steps, repeated
frames = torch.from_numpy(host).cuda().reshape(rendered, C, H, W).repeat(T // rendered, 1, 1, 1).reshape(-1, H, W).contiguous()
T = frames.shape[0] // C
torch.cuda.synchronize()

legs = {"none": None} if args.baseline_only else {"none": None, "subpixel": SUBPIX}
trackers = {}
for name, sp in legs.items():
    kw = {} if sp is None else {"subpixel": sp}
    trackers[name] = BatchTracker(K, dist, R, t, F, W, H, T, max_points=wl.max_points, max_groups=wl.max_groups, depth=3, **kw)
    for _ in range(4):
        trackers[name].step(frames)
    trackers[name].synchronize()

ms = {name: [] for name in legs}
for _ in range(args.rounds):
    for name, trk in trackers.items():  # alternating: whatever drifts (clocks, the box's other tenants) hits both legs alike
        t0 = time.perf_counter()
        for _ in range(args.steps):
            trk.step(frames)
        trk.synchronize()
        ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)

res = {"config": f"{C} x {W}x{H}, {args.markers} markers, {T} time steps per batch, depth 3, {args.steps} batches per run, {args.rounds} runs per leg",
       "ms_per_step": {k: round(statistics.median(v), 4) for k, v in ms.items()},
       "ms_per_step_runs": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
if not args.baseline_only:
    res["subpixel_over_none"] = round(res["ms_per_step"]["subpixel"] / res["ms_per_step"]["none"], 4)
    # the kernel alone: one batch at a time, the refine launch between two events
    trk = BatchTracker(K, dist, R, t, F, W, H, T, max_points=wl.max_points, max_groups=wl.max_groups, depth=1)
    ctx, records = trk.ctx, trk.extract(frames)
    out, kern = None, []
    for i in range(12):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        trk.extract(frames)  # the blob stage in front of it, as in the pipeline
        a.record()
        out = ctx.refine_centroids(frames, records, cam_mod=C, max_blobs=wl.max_points, coords="ideal", out=out, **SUBPIX)
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            kern.append(a.elapsed_time(b))
    cnt = records[:, 0]
    flags = out["flags"][torch.arange(out["flags"].shape[1], device="cuda")[None, :] < cnt[:, None]]
    res["refine_kernel_ms"] = round(statistics.median(kern), 4)
    res["refine_kernel_ms_runs"] = [round(x, 4) for x in kern]
    res["points_refined"] = int(flags.numel())
    res["points_flagged_fallback"] = int((flags & 15).ne(0).sum())
print(json.dumps(res))
