#!/usr/bin/env python3
"""Time of mocap_rig_bundle_adjust on the noisy16 case of tests/rig_ba_ref.py scaled to 20 000 wand points (one-off
measurement, numbers in DESIGN.md section 5 and profiles/README.md).  The problem stays resident on the GPU; a call is timed
with device events after a warm-up, for max_iters = 50 (the default: every iteration is enqueued, those after the stop return
at once) and for max_iters = the iterations the loop actually needs, which prices the enqueue-everything design against a
host that would stop launching, and for max_iters = 1 (one iteration with its init and finish launches).  --loss-scale C times
mocap_rig_bundle_adjust_robust with the Cauchy loss of scale C px and both per-observation outputs in its place.
--intrinsics times mocap_rig_bundle_adjust_intrinsics on the same problem and start: the context's K and dist as kd, every
lens parameter of every camera free (mask 0x1ff), the loss of --loss-scale or none.  Also prints the NumPy restatement's CPU
time for the same problem (--numpy, the plain loop).

  python scratch/time_rig_ba.py [--points 20000] [--reps 5] [--loss-scale 2.0] [--intrinsics] [--numpy]
  rocprofv3 --kernel-trace --stats -d DIR -- python scratch/time_rig_ba.py --reps 2     (kernel split, a run of its own)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loss-scale", type=float, default=None)
    ap.add_argument("--intrinsics", action="store_true")
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()
    import torch

    import rig_ba_ref as rb
    from mocapv2_amd.engine import MocapContext
    c = rb.case("noisy16", args.points)
    prob = c["prob"]
    R, t, X = rb.perturbed_start(c, rb.START_SEED["noisy16"])
    off, cam, uv = prob.point_major()
    ctx = MocapContext(1, 1)
    ctx.set_cameras(prob.K, prob.dist, R, t)
    dev = ctx.device
    poses = np.c_[R.reshape(-1, 9), t]
    d_off, d_cam, d_uv = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (off, cam, uv))
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    per_obs = torch.zeros((2, len(cam)), dtype=torch.float64, device=dev)
    kd = np.c_[prob.K[:, 0, 0], prob.K[:, 1, 1], prob.K[:, 0, 2], prob.K[:, 1, 2], prob.dist]
    masks = np.full(prob.C, 0x1FF, np.int32)

    def call(max_iters):
        d_poses, d_pts, d_kd = torch.from_numpy(poses).to(dev), torch.from_numpy(X).to(dev), torch.from_numpy(kd).to(dev)
        hist = torch.zeros((max_iters, 4), dtype=torch.float64, device=dev)
        res = torch.zeros(4, dtype=torch.float64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        if args.intrinsics:
            robust = args.loss_scale is not None
            rc = ctx.lib.mocap_rig_bundle_adjust_intrinsics(ctx._h, prob.C, prob.N, len(cam), p(d_off), p(d_cam), p(d_uv), p(d_kd),
                                                            masks.ctypes.data_as(C.POINTER(C.c_int)), p(d_poses), p(d_pts), max_iters, 1e-12,
                                                            1e-3, p(hist), p(res), int(robust), args.loss_scale or 0.0,
                                                            p(per_obs[0]) if robust else None, p(per_obs[1]) if robust else None, stream)
        elif args.loss_scale is None:
            rc = ctx.lib.mocap_rig_bundle_adjust(ctx._h, prob.C, prob.N, len(cam), p(d_off), p(d_cam), p(d_uv), p(d_poses), p(d_pts),
                                                 max_iters, 1e-12, 1e-3, p(hist), p(res), stream)
        else:
            rc = ctx.lib.mocap_rig_bundle_adjust_robust(ctx._h, prob.C, prob.N, len(cam), p(d_off), p(d_cam), p(d_uv), p(d_poses),
                                                        p(d_pts), max_iters, 1e-12, 1e-3, p(hist), p(res), 1, args.loss_scale,
                                                        p(per_obs[0]), p(per_obs[1]), stream)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, ctx.lib.mocap_last_error()
        return e0.elapsed_time(e1), res.cpu().numpy()

    _, res = call(50)  # warm-up: code objects, scratch
    iters = int(res[1])
    out = {"points": prob.N, "observations": len(cam), "cameras": prob.C, "intrinsics": args.intrinsics, "loss_scale": args.loss_scale, "status": int(res[0]),
           "iterations": iters, "rms_px": float(np.sqrt(res[3] / len(cam)))}
    for name, mi in (("ms_max_iters_50", 50), ("ms_max_iters_needed", max(iters, 1)), ("ms_max_iters_1", 1)):
        ms = [call(mi)[0] for _ in range(args.reps)]
        out[name] = {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}
    if args.numpy:
        t0 = time.perf_counter()
        ref = rb.lm(prob, R, t, X)
        out["numpy_restatement_s"] = time.perf_counter() - t0
        out["numpy_iterations"] = ref["iterations"]
        out["cost_ratio_minus_1"] = float(res[3] / ref["cost"] - 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
