#!/usr/bin/env python3
"""Time of mocap_refine_points beside mocap_correspond_visible, whose outputs it reads (one-off measurement, numbers in DESIGN.md
section 4 and profiles/README.md).  Points come from tests/correspond_visible_ref.scene_case (ring rig in 1920 x 1080, 0.5 px
jitter, one seed per time step), as in scratch/time_correspond_visible.py; the refinement runs in its indexed form on the
correspondence's own rows, with the trackers' defaults (max_iters 10, ftol 1e-9, lambda0 1e-3), without and with pruning.  Every
call is timed with device events after a warm-up; all in one process, one after the other.

  python scratch/time_refine_points.py [--steps 512] [--reps 7]
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
    fn()  # warm-up: code objects
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
    args = ap.parse_args()
    import torch

    import correspond_visible_ref as cv
    from mocapv2_amd.engine import MocapContext
    T = args.steps
    out = {"steps": T, "reps": args.reps, "configs": []}
    for C, M, p in CONFIGS:
        cases = [cv.scene_case(C, M, p, seed) for seed in range(T)]
        K, dist, R, t = cv.scene_arrays(cases[0][0])
        pts = torch.from_numpy(np.stack([c[1] for c in cases])).cuda()
        counts = torch.from_numpy(np.stack([c[2] for c in cases]).astype(np.int32)).cuda()
        ctx = MocapContext(1, 1)
        ctx.set_cameras(K, dist, R, t)
        res = ctx.correspond_visible(pts, counts)
        torch.cuda.synchronize()
        n = res["n"].cpu().numpy()
        assert (n >= 0).all(), n.min()
        kw = dict(views=res["views"], pts=pts, idx=res["idx"])
        ref = ctx.refine_points(res["xyz"], res["n"], **kw)
        torch.cuda.synchronize()
        live = (np.arange(ref["status"].shape[1])[None, :] < n[:, None])
        status, iters = ref["status"].cpu().numpy()[live], ref["iters"].cpu().numpy()[live]
        assert (status > 0).all()
        row = {"cameras": C, "markers": M, "p_hidden": p, "rows": int(live.sum()), "rows_per_step_buffer": int(ref["status"].shape[1]),
               "iterations_mean": float(iters.mean()), "iterations_max": int(iters.max()),
               "stops": np.bincount(status, minlength=5).tolist(),
               "correspond_visible_ms": timed(lambda: ctx.correspond_visible(pts, counts, out=res), args.reps),
               "refine_points_ms": timed(lambda: ctx.refine_points(res["xyz"], res["n"], out=ref, **kw), args.reps),
               "refine_points_pruning_ms": timed(lambda: ctx.refine_points(res["xyz"], res["n"], out=ref, max_res2=9.0, max_drop=1, **kw),
                                                 args.reps)}
        row["ratio_to_correspond_visible"] = row["refine_points_ms"]["median"] / row["correspond_visible_ms"]["median"]
        out["configs"].append(row)
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
