#!/usr/bin/env python3
"""Time of one MocapContext.learn_rigid_bodies call on a long take against the NumPy restatement (tests/rigid_learn_ref.py) on the
same arrays: T = 36 000 steps (ten minutes at 60 Hz), 16 bodies of 4 markers = K = 64 identities, G = 16 groups, 10 % of the markers
hidden, 4 clutter points per step.  HIP events around warm calls, the median of `--reps`; also the two device calls on their own.
   python scratch/time_rigid_learn.py [--steps 36000] [--reps 9] [--no-ref]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import rigid_learn_ref as rl  # noqa: E402
import rigid_ref as rr  # noqa: E402
from mocapv2_amd.engine import MocapContext  # noqa: E402


def long_take(T, B=16, M=4, hidden=0.1, clutter=4, seed=1):
    rng = np.random.default_rng(seed)
    models = np.stack([rr.make_body(rng, M) for _ in range(B)])
    q = rng.normal(size=(T, B, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    w, x, y, z = (q[..., k] for k in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1).reshape(T, B, 3, 3)
    pts = np.einsum("tbuv,bpv->tbpu", R, models) + rng.uniform(-1, 1, (T, B, 1, 3)) + rng.normal(scale=rr.NOISE, size=(T, B, M, 3))
    Q = B * M + clutter
    xyz = np.concatenate([pts.reshape(T, B * M, 3), rng.uniform(-1.2, 1.2, (T, clutter, 3))], axis=1)
    ident = np.concatenate([np.broadcast_to((10 * np.arange(B)[:, None] + np.arange(M)[None, :]).reshape(-1), (T, B * M)),
                            1000 + np.arange(T * clutter).reshape(T, clutter)], axis=1).astype(np.int32)
    ident[:, :B * M][rng.random((T, B * M)) < hidden] = -1  # a hidden marker: its row holds no track
    perm = np.argsort(rng.random((T, Q)), axis=1)
    rows = np.arange(T)[:, None]
    return np.ascontiguousarray(xyz[rows, perm]), np.full(T, Q, np.int32), np.ascontiguousarray(ident[rows, perm]), models


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=36000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    xyz, n, ident, models = long_take(a.steps)
    ctx = MocapContext(1, 1)
    dev = tuple(torch.from_numpy(v).cuda() for v in (xyz, n, ident))
    kw = dict(spread=rl.SPREAD, min_steps=100)
    res = ctx.learn_rigid_bodies(*dev, **kw)
    K, G = len(res["ids"]), len(res["members"])
    err = max(rl.aligned_error(m, models[g]).max() for g, m in enumerate(res["models"]))
    print(f"T = {a.steps}, K = {K}, G = {G}, status {sorted(set(res['status'].tolist()))}, worst learned point {err * 1e3:.4f} mm", flush=True)
    print(f"learn_rigid_bodies : {median_ms(lambda: ctx.learn_rigid_bodies(*dev, **kw), a.reps):9.3f} ms (ids found on the host, tables read back, grouping)")
    print(f"  with ids given   : {median_ms(lambda: ctx.learn_rigid_bodies(*dev, ids=res['ids'], **kw), a.reps):9.3f} ms")
    print(f"marker_pair_stats  : {median_ms(lambda: ctx.marker_pair_stats(*dev, res['ids']), a.reps):9.3f} ms")
    print(f"rigid_learn        : {median_ms(lambda: ctx.rigid_learn(*dev, res['members']), a.reps):9.3f} ms", flush=True)
    if not a.no_ref:
        t0 = time.perf_counter()
        pairs = rl.pair_stats(xyz, n, ident, res["ids"])
        t1 = time.perf_counter()
        want = rl.rigid_learn(xyz, n, ident, res["members"])
        t2 = time.perf_counter()
        same = all(np.array_equal(np.ascontiguousarray(pairs[k]).view(np.uint8), np.ascontiguousarray(res["pairs"][k]).view(np.uint8)) for k in pairs)
        same = same and all(np.array_equal(want["model"][g, :len(m)].view(np.uint64), m.view(np.uint64)) for g, m in enumerate(res["models"]))
        print(f"restatement        : pair_stats {t1 - t0:.2f} s, rigid_learn {t2 - t1:.2f} s, together {t2 - t0:.2f} s; the same bits: {same}")


if __name__ == "__main__":
    main()
