#!/usr/bin/env python3
"""Time of mocap_correspond_visible against the two figures that decide what visibility="any" costs (one-off measurement,
numbers in DESIGN.md section 4 and profiles/README.md): the frame -> centroid time of the same batch (stage A, which stage B
has to hide behind in the pipelined tracker) and mocap_correspond on the same points (full visibility only: with hidden
views that call reports nothing).  Points come from tests/correspond_visible_ref.scene_case (ring rig in 1920 x 1080, 0.5 px
jitter, one seed per time step), frames from synth.Scene.render_batch (a few rendered time steps repeated to T on the
device).  Every call is timed with device events after a warm-up; all in one process, one after the other.

  python scratch/time_correspond_visible.py [--steps 512] [--reps 7] [--frame-steps 4]
  rocprofv3 --kernel-trace --stats -d DIR -- python scratch/time_correspond_visible.py --reps 2     (a run of its own)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = [(6, 8, 0.0), (6, 8, 0.3), (6, 32, 0.0), (6, 32, 0.3)]  # cameras, markers, probability that a view is hidden


def timed(fn, reps):
    import torch
    fn()  # warm-up: code objects, scratch
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frame-steps", type=int, default=4)
    args = ap.parse_args()
    import torch

    import correspond_visible_ref as cv
    from mocapv2_amd.engine import MocapContext
    from mocapv2_amd.synth import MILD_DIST, Scene
    T, W, H = args.steps, 1920, 1080
    out = {"steps": T, "reps": args.reps, "configs": []}
    for C, M, p in CONFIGS:
        cases = [cv.scene_case(C, M, p, seed) for seed in range(T)]
        scene = cases[0][0]
        K, dist, R, t = cv.scene_arrays(scene)
        pts = torch.from_numpy(np.stack([c[1] for c in cases])).cuda()
        counts = torch.from_numpy(np.stack([c[2] for c in cases]).astype(np.int32)).cuda()
        ctx = MocapContext(W, H, n_slots=C)
        ctx.set_cameras(K, dist, R, t)
        ctx.set_fundamentals(np.stack(scene.Fs))
        res = ctx.correspond_visible(pts, counts)
        torch.cuda.synchronize()
        n = res["n"].cpu().numpy()
        assert (n >= 0).all(), n.min()
        row = {"cameras": C, "markers": M, "p_hidden": p, "markers_found_per_step": float(n.mean()),
               "correspond_visible_ms": timed(lambda: ctx.correspond_visible(pts, counts, out=res), args.reps)}
        one = ctx.correspond_visible(pts, counts, max_passes=1)
        row["correspond_visible_one_pass_ms"] = timed(lambda: ctx.correspond_visible(pts, counts, max_passes=1, out=one), args.reps)
        if p == 0.0:
            old = ctx.correspond(pts, counts)
            row["correspond_ms"] = timed(lambda: ctx.correspond(pts, counts, out=old), args.reps)
            row["ratio_to_correspond"] = row["correspond_visible_ms"]["median"] / row["correspond_ms"]["median"]
        # stage A of the same batch: T x C frames with M discs each, through the lens the bench uses
        lens = Scene(C, W, H, dist=MILD_DIST)
        for c in range(C):
            ctx.set_undistort(c, lens.K, lens.dist)
        few = torch.from_numpy(lens.render_batch(seed=900, n_steps=args.frame_steps, n_markers=M, radius_range=(16, 22))).cuda()
        frames = few.repeat((T + args.frame_steps - 1) // args.frame_steps, 1, 1, 1)[:T].reshape(T * C, H, W).contiguous()
        records = ctx.blob_centroids(frames, cam_mod=C, max_blobs=max(32, M))
        row["frames_to_centroids_ms"] = timed(lambda: ctx.blob_centroids(frames, cam_mod=C, max_blobs=max(32, M), records=records), args.reps)
        row["hides_behind_stage_a"] = row["correspond_visible_ms"]["median"] < row["frames_to_centroids_ms"]["median"]
        out["configs"].append(row)
        del frames, few
        ctx.close()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
