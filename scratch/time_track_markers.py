#!/usr/bin/env python3
"""Time of mocap_track_markers beside the two figures that decide what identities cost (one-off measurement, numbers in
DESIGN.md section 4 and profiles/README.md): mocap_correspond_visible on the same batch (whose xyz and n the tracker reads as
they are) and the frame -> centroid time of that batch (stage A, which stage B has to hide behind in the pipelined tracker).
The batch is scratch/time_correspond_visible.py's rigs (ring rig in 1920 x 1080, 0.5 px jitter, every view hidden with probability
p, lists shuffled) with one difference: the markers of consecutive time steps belong together -- they follow the smooth paths of
tests/track_ref.scene (largest step 30 mm), so that tracks live as they do in a recording.  Frames come from
synth.Scene.render_batch.  Every call is timed with device events after a
warm-up, all in one process, one after the other.  The tracker is timed with max_tracks = 64 (two waves, the fewest the kernel
runs with) and 256 (four waves) and, for the per-phase split, on inputs that switch phases off: no detections at all (staging, stores and
the step's barriers), and a gate nothing passes (+ the candidate scan, no rounds beyond the first, every detection a birth).

  python scratch/time_track_markers.py [--steps 512] [--reps 7] [--frame-steps 4]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_correspond_visible import CONFIGS, timed  # noqa: E402  (the same rigs, the same clock)

GATE = 0.05


def moving_points(scene, C, M, p, T, seed=0):
    """pts [T, C, M, 2] float64, counts [T, C] int32: the views of M markers on track_ref.scene's paths, as scene_case lays them out"""
    import track_ref as tr
    rng = np.random.default_rng(seed)
    path = tr.scene(seed, 0.8, T=T, markers=M, Q=M + 1)[4] - 0.5  # the rig looks at the cube around the origin
    pts = np.zeros((T, C, M, 2))
    counts = np.zeros((T, C), np.int32)
    for c in range(C):
        px = scene.pixels(path.reshape(T * M, 3), c, distorted=False).reshape(T, M, 2) + rng.normal(0, 0.5, (T, M, 2))
        for t in range(T):
            rows = px[t][rng.random(M) >= p]
            pts[t, c, :len(rows)] = rows[rng.permutation(len(rows))]
            counts[t, c] = len(rows)
    return pts, counts


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
    out = {"steps": T, "reps": args.reps, "gate": GATE, "configs": []}
    for C, M, p in CONFIGS:
        scene = cv.scene_case(C, M, p, 0)[0]
        K, dist, R, t = cv.scene_arrays(scene)
        pts, counts = (torch.from_numpy(a).cuda() for a in moving_points(scene, C, M, p, T))
        ctx = MocapContext(W, H, n_slots=C)
        ctx.set_cameras(K, dist, R, t)
        res = ctx.correspond_visible(pts, counts)
        torch.cuda.synchronize()
        n = res["n"].cpu().numpy()
        assert (n >= 0).all(), n.min()
        row = {"cameras": C, "markers": M, "p_hidden": p, "markers_found_per_step": float(n.mean()), "rows_per_step": int(res["xyz"].shape[1]),
               "correspond_visible_ms": timed(lambda: ctx.correspond_visible(pts, counts, out=res), args.reps)}

        def track_ms(max_tracks, xyz, cnt, gate=GATE):
            state = ctx.track_state(max_tracks)
            ids = ctx.track_markers(xyz, cnt, state, gate)
            ms = timed(lambda: ctx.track_markers(xyz, cnt, state, gate, out=ids), args.reps)
            ms["us_per_step"] = 1e3 * ms["median"] / T
            return ms, ids

        row["track_ms"], ids = track_ms(64, res["xyz"], res["n"])
        row["track_256_slots_ms"], _ = track_ms(256, res["xyz"], res["n"])
        status = ids["status"].cpu().numpy()
        row["steps_with_a_code"] = int((status != 0).sum())
        row["tracked_rows_per_step"] = float((ids["id"].cpu().numpy() >= 0).sum() / T)
        # the split: nothing to scan; scans and births without matches
        row["track_no_detections_ms"], _ = track_ms(64, res["xyz"], torch.zeros_like(res["n"]))
        row["track_no_candidates_ms"], _ = track_ms(64, res["xyz"], res["n"], gate=1e-9)
        # stage A of the same batch: T x C frames with M discs each, through the lens the bench uses
        lens = Scene(C, W, H, dist=MILD_DIST)
        for c in range(C):
            ctx.set_undistort(c, lens.K, lens.dist)
        few = torch.from_numpy(lens.render_batch(seed=900, n_steps=args.frame_steps, n_markers=M, radius_range=(16, 22))).cuda()
        frames = few.repeat((T + args.frame_steps - 1) // args.frame_steps, 1, 1, 1)[:T].reshape(T * C, H, W).contiguous()
        records = ctx.blob_centroids(frames, cam_mod=C, max_blobs=max(32, M))
        row["frames_to_centroids_ms"] = timed(lambda: ctx.blob_centroids(frames, cam_mod=C, max_blobs=max(32, M), records=records), args.reps)
        # the requirement of DESIGN.md section 4 for stage B: correspondence + identities below stage A of the same batch, by more
        # than the spread of the calls (the worst of B against the best of A)
        b = row["correspond_visible_ms"]
        k = row["track_ms"]
        row["stage_b_median_ms"] = b["median"] + k["median"]
        row["hides_behind_stage_a"] = b["max"] + k["max"] < row["frames_to_centroids_ms"]["min"]
        out["configs"].append(row)
        del frames, few
        ctx.close()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
