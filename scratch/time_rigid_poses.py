#!/usr/bin/env python3
"""Time of mocap_rigid_poses (one-off measurement, numbers in DESIGN.md section 4): T = 512 time steps, B = 2 bodies of 4 markers
each (tests/rigid_ref.rigid_scene: random poses, 0.5 mm noise, rows shuffled, nothing hidden), with 8 detections per step (the two
bodies alone) and with 32 (24 stray points beside them); tol = 3 mm, gate = 6 mm, min_markers = 3, max_hyp = 1024.  Every call is
timed with a pair of device events after a warm-up, one call after the other in one process; median of `--reps` calls (min - max).
Also printed: the candidates per (step, body) the restatement counts on the first 16 steps, which is what the time follows.

  python scratch/time_rigid_poses.py [--steps 512] [--reps 21]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_correspond_visible import timed  # noqa: E402  (the same clock)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    import torch

    import rigid_ref as rr
    from mocapv2_amd.engine import MocapContext
    T = args.steps
    ctx = MocapContext(1, 1)
    out = {"steps": T, "bodies": 2, "reps": args.reps, "tol": rr.TOL, "gate": rr.GATE, "configs": []}
    for clutter in (0, 24):
        sc = rr.rigid_scene(0, T=T, sizes=(4, 4), hidden=0.0, clutter=clutter, Q=32)
        xyz, n = torch.from_numpy(sc["xyz"]).cuda(), torch.from_numpy(sc["n"]).cuda()
        bodies = ctx.rigid_bodies(sc["models"], rr.MIN_AREA)
        res = ctx.rigid_poses(xyz, n, bodies, rr.TOL, rr.GATE)
        torch.cuda.synchronize()
        status = res["status"].cpu().numpy()
        tri = [rr.triples_of(m, rr.MIN_AREA) for m in sc["models"]]
        cands = [rr.solve_body(sc["xyz"][s, :sc["n"][s]], sc["models"][b], tri[b], rr.TOL, rr.GATE, 3, 1024).get("n_cand", 0)
                 for s in range(min(T, 16)) for b in range(2)]
        row = {"detections_per_step": int(sc["n"][0]), "found": int((status == 0).sum()), "of": int(status.size),
               "candidates_per_step_and_body": {"mean": float(np.mean(cands)), "max": int(max(cands))},
               "rigid_poses_ms": timed(lambda: ctx.rigid_poses(xyz, n, bodies, rr.TOL, rr.GATE, out=res), args.reps)}
        row["us_per_step"] = 1e3 * row["rigid_poses_ms"]["median"] / T
        out["configs"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
