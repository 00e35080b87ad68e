#!/usr/bin/env python3
"""Time of mocap_fundamental_ransac at the sizes a 16-camera rig gives (one-off measurement, numbers in profiles/README.md):
  large      15 pairs (0 -> i), 20 000 points each, 30 % outliers, H = 2048
  all-pairs  120 pairs (i -> j, i < j), the same per pair
Inputs stay resident on the GPU; the call is timed with device events after a warm-up, the matrices it returns are checked
to be finite.  FP64 operations are counted from the shapes: one point-against-hypothesis evaluation is 42 separately rounded
multiplications and additions (fundamental.hip: is_inlier); the library is built without fused multiply-add, so the rate
to compare with is the FP64 vector INSTRUCTION rate, half the datasheet's FMA-counted 78.6 TFLOPS.

  python scratch/time_fundamental.py [--reps 10] [--numpy] [--only large|all]
  rocprofv3 --kernel-trace --stats -d DIR -- python scratch/time_fundamental.py --reps 3     (kernel split, a run of its own)
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

OPS_PER_EVALUATION = 42          # 24 multiplications and 18 additions (fundamental.hip: is_inlier)
FP64_VECTOR_FMA_TFLOPS = 78.6    # MI355X datasheet, an FMA counted as two
FP64_VECTOR_OPS_T = FP64_VECTOR_FMA_TFLOPS / 2  # separately rounded operations per second (x 1e12)


def batch(pairs, n_points, H):
    import fundamental_ref as fr
    from mocapv2_amd.calibrate import sample_table
    from mocapv2_amd.synth import Scene
    sc = Scene(16)
    a, b, s = [], [], []
    for k, (i, j) in enumerate(pairs):
        pa, pb = fr.synthetic_pair(sc, i, j, n_points, 40 + k, 0.30)[:2]
        a.append(pa)
        b.append(pb)
        s.append(sample_table(n_points, H, 40 + k))
    return np.concatenate(a), np.concatenate(b), np.stack(s), np.arange(len(pairs) + 1, dtype=np.int32) * n_points


def time_batch(ctx, name, pairs, n_points, H, reps):
    import torch
    a, b, s, off = batch(pairs, n_points, H)
    P = len(pairs)
    dev = ctx.device
    d_a, d_b, d_s = (torch.from_numpy(x).to(dev) for x in (a, b, s))
    F_s = torch.zeros((P, 9), dtype=torch.float64, device=dev)
    F_r = torch.zeros((P, 9), dtype=torch.float64, device=dev)
    mask = torch.zeros(P * n_points, dtype=torch.uint8, device=dev)
    status = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = ctx.lib.mocap_fundamental_ransac(ctx._h, P, p(d_a), p(d_b), off.ctypes.data_as(C.POINTER(C.c_int)), p(d_s), H, 3.0, 1,
                                              p(F_s), p(F_r), p(mask), p(status), None, stream)
        assert rc == 0, ctx.lib.mocap_last_error()

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    st = status.cpu().numpy()
    assert (st[:, 0] >= 0).all() and torch.isfinite(F_r).all()
    evaluations = P * H * n_points
    ops = evaluations * OPS_PER_EVALUATION
    med = float(np.median(ms))
    out = {"batch": name, "pairs": P, "points_per_pair": n_points, "hypotheses": H, "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
           "ms_max": round(max(ms), 3), "reps": reps, "evaluations": evaluations, "fp64_ops_scoring": ops,
           "scoring_tops_over_call_time": round(ops / (med * 1e-3) / 1e12, 3),
           "share_of_fp64_vector_instruction_peak": round(ops / (med * 1e-3) / 1e12 / FP64_VECTOR_OPS_T, 4),
           "inliers_min_max": [int(st[:, 1].min()), int(st[:, 1].max())]}
    print(json.dumps(out), flush=True)
    return (a[:n_points], b[:n_points], s[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy", action="store_true", help="also time the NumPy restatement on ONE pair on this host (about 5 s)")
    ap.add_argument("--only", choices=["large", "all"], default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    from mocapv2_amd.engine import MocapContext
    ctx = MocapContext(1, 1)
    one = None
    if args.only in (None, "large"):
        one = time_batch(ctx, "large", [(0, i) for i in range(1, 16)], 20000, 2048, args.reps)
    if args.only in (None, "all"):
        time_batch(ctx, "all-pairs", [(i, j) for i in range(16) for j in range(i + 1, 16)], 20000, 2048, args.reps)
    if args.numpy and one is not None:
        import fundamental_ref as fr
        t0 = time.time()
        r = fr.ransac(one[0], one[1], one[2], 3.0)
        print(json.dumps({"numpy_one_pair_s": round(time.time() - t0, 2), "inliers": r["n_inliers"]}), flush=True)


if __name__ == "__main__":
    main()
