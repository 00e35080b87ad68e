"""The step control of the two device solvers (csrc/lm.h under csrc/rig_ba.hip and csrc/intrinsics.hip) off the happy path:
steps rejected by the gain ratio, steps rejected for a point behind a camera, failed factorisations, the stops on max_iters,
lambda and two failed solves, and the state handed back when a loop ends on rejected steps.  Every run is a case of
tests/lm_cases.py, walked against the restatement (tests/lm_ref.py's control); tests/test_lm_branches_host.py establishes on
the restatement alone that each case takes its branches far from every decision boundary, and prints the spreads quoted here.

The allowance of a history column is the project's: 8 x the restatement's own largest spread of that column under 10 seeded
permutations of the order of the sums, 1e-12 where that spread is 0 -- measured on the restatement, never on the kernels.

Not here: a single failed solve followed by a solved step, in either loop.  No run was found whose failed solve holds under
permutation of the sums and whose next solve succeeds (test_lm_branches_host.py::test_the_table_covers_every_branch says
why), so that the clearing of chol_fail after one failure is not walked: every failed solve below is followed by another.  For
the intrinsics loop about 100 harsh starts and the starts of lm_cases gave no 6x6 or 9x9 factorisation that fails with a pivot
below -1e-6 of the diagonal; its failed solves here are the structural ones of lm_cases.singular_camera (a view whose corners
all sit at the board's origin: the first pivot of its V* is exactly 0)."""
import numpy as np
import pytest

import intrinsics_ref as ir
import lm_cases as lc
import rig_ba_ref as rb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mocapv2_amd.engine import MocapContext
    return MocapContext(1, 1)


def poses12(R, t):
    return np.c_[np.asarray(R, float).reshape(len(R), 9), np.asarray(t, float).reshape(len(R), 3)]


# ---- what holds of any history by the rule alone: no tolerance --------------------------------------------------------------------
def check_exact_history(h, cost_initial, failed):
    """h: the device's history [iterations][4]; failed [iterations]: the solve failed (from the restatement, whose accept
    sequence the caller has found equal).  A rejected or failed iteration leaves the cost as it was, bit for bit; after j
    non-accepts in a row the next row's lambda is the first rejected row's times 2^(j (j + 1) / 2), exactly (powers of two); a
    failed solve has |step| = 0 and a solved one has not."""
    acc = h[:, 2] > 0
    assert set(h[:, 2].tolist()) <= {0.0, 1.0}
    first = None
    for i in range(len(h)):
        if acc[i]:
            first = None
            continue
        assert h[i, 0] == (h[i - 1, 0] if i else cost_initial), ("cost after a rejection", i)
        first = i if first is None else first
        j = i - first + 1
        if i + 1 < len(h):
            assert h[i + 1, 1] == h[first, 1] * 2.0 ** (j * (j + 1) // 2), ("lambda after rejections", i, j)
    assert (h[failed, 3] == 0).all() and (h[~failed, 3] > 0).all()


def walk(name, h, status, iterations, cost_initial, base, spread):
    """The device's history against the restatement run `base`: decisions equal, columns within their allowance, and the exact
    properties.  Prints the restatement's spread and the measured difference of each column."""
    ref = base["history"]
    print(f"{name}: iterations {iterations} / {base['iterations']}  status {status} / {base['status']}  accepted "
          f"{''.join('1' if a else '0' for a in h[:, 2])} / {lc.sequence(base)}")
    assert iterations == base["iterations"] == len(h) and status == base["status"]
    assert np.array_equal(h[:, 2], ref[:, 2])
    diffs = {}
    for k, col in (("cost", 0), ("lambda", 1), ("step", 3)):
        a, b = ref[:, col], h[:, col]
        diffs[k] = float(np.where(a == 0, np.abs(b), np.abs(b / np.where(a == 0, 1.0, a) - 1)).max())
        print(f"{name} {k}: restatement's spread {float(np.max(spread[k])):.3e}  GPU - restatement {diffs[k]:.3e}  allowed {lc.allowance(spread, k):.3e}")
    for k in diffs:
        assert diffs[k] <= lc.allowance(spread, k), (name, k)
    assert abs(cost_initial / base["cost_initial"] - 1) < 1e-12
    check_exact_history(h, cost_initial, np.isnan(base["rho"]))


def state_difference(name, got, ref, spread, keys):
    """Returned arrays against the restatement's, each relative to its largest entry, within 8 x the restatement's spread"""
    for k in keys:
        d = float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max())
        print(f"{name} {k}: restatement's spread {spread[k]:.3e}  GPU - restatement {d:.3e}  allowed {lc.allowance(spread, k):.3e}")
    for k in keys:
        assert np.abs(got[k] - ref[k]).max() <= lc.allowance(spread, k) * np.abs(ref[k]).max(), (name, k)


# ---- the rig ----------------------------------------------------------------------------------------------------------------------
def rig_run(ctx, name, max_iters=None):
    c = lc.rig_case(name)
    prob, (R, t, X) = c["prob"], c["start"]
    kw = dict(c["kw"], max_iters=c["kw"]["max_iters"] if max_iters is None else max_iters)
    if c["loss_c"] is not None:
        kw.update(loss="cauchy", loss_scale=c["loss_c"])
    ctx.set_cameras(prob.K, prob.dist, R, t)
    return ctx.rig_bundle_adjust(*prob.point_major(), poses12(R, t), X, **kw)


@pytest.mark.parametrize("name", list(lc.RIG))
def test_rig_loop_walks_the_restatement_through_rejections_and_failed_solves(ctx, name):
    """Cases A-D, F, G9, G22 of lm_cases.RIG: 6 cameras, 95 points in one workgroup (G9, G22: 295 in two, so the partials of the trial
    cost are summed over two blocks and the point-behind flag is raised from either); F under the Cauchy loss.  Equal:
    iterations, status, the accepted column.  Within 8 x the restatement's spread: cost, lambda, |step| per iteration.  Exact:
    check_exact_history.
    Restatement's spread (CPU), cost / lambda / |step|        GPU - restatement (MI355X)
      A    6.4e-13 / 1.0e-12 / 4.9e-09                         3.3e-13 / 8.6e-13 / 3.1e-09   (14 iterations, ftol)
      B    1.0e-07 / 8.7e-08 / 3.8e-07                         2.0e-09 / 1.5e-09 / 9.8e-09   (16, ftol)
      C    3.0e-08 / 2.1e-08 / 5.2e-08                         2.1e-08 / 1.5e-08 / 2.5e-08   (11, max_iters)
      D    3.3e-16 / 0 / 0                                     1.1e-16 / 0 / 0               (2, Cholesky)
      F    9.5e-12 / 2.9e-11 / 2.9e-07                         2.0e-12 / 1.4e-11 / 2.2e-07   (25, ftol)
      G9   1.4e-11 / 6.5e-12 / 5.0e-09                         8.7e-13 / 8.0e-13 / 3.1e-10   (16, ftol)
      G22  1.2e-09 / 1.0e-09 / 1.2e-08                         5.1e-10 / 3.9e-10 / 5.1e-10   (20, ftol)"""
    base, same, spread = lc.rig_reference(name)
    assert same
    got = rig_run(ctx, name)
    walk(name, got["history"], got["status"], got["iterations"], got["cost_initial"], base, spread)
    assert got["cost"] == got["history"][-1, 0]


@pytest.mark.parametrize("name", ["A", "F", "G9"])
def test_rig_state_after_trailing_rejections_is_the_last_accepted_one(ctx, name):
    """A run cut at max_iters = k, right after the accepted iteration k - 1, and a run cut at k + j, after the j rejected steps
    that follow it (A: k = 1, j = 3; F, under the loss: 12, 2; G9, two workgroups: 3, 2), hand back the same bits: poses,
    points, cost, and under the loss every observation's error and weight (rig_residuals_kernel reads the arrays handed back).
    The rejected trial states never leave the device.
    That state against the restatement's, relative to the largest entry, poses / points:
      restatement's spread (CPU)  A 5.9e-14 / 1.0e-13   F 3.1e-12 / 3.1e-12   G9 9.9e-14 / 8.6e-14
      GPU - restatement (MI355X)  A 1.0e-14 / 1.1e-14   F 1.2e-12 / 1.2e-12   G9 1.0e-14 / 1.7e-14"""
    base = lc.rig_reference(name)[0]
    k, j = lc.trailing_rejections(base, 6 if name == "F" else 0)
    short, long = rig_run(ctx, name, k), rig_run(ctx, name, k + j)
    ref, same, spread = lc.rig_reference(name, k + j)
    assert same and lc.sequence(ref)[k - 1:] == "1" + "0" * j
    assert short["iterations"] == k and long["iterations"] == k + j and short["status"] == long["status"] == rb.STOP_MAX_ITERS
    assert np.array_equal(long["history"][:, 2], ref["history"][:, 2]) and long["history"][:k].tobytes() == short["history"].tobytes()
    keys = ("poses", "points") + (("obs_err", "obs_weight") if lc.rig_case(name)["loss_c"] is not None else ())
    for key in keys:
        assert short[key].tobytes() == long[key].tobytes(), key
    assert short["cost"] == long["cost"]
    state_difference(name, {"poses": long["poses"][1:], "points": long["points"]},
                     {"poses": poses12(ref["R"], ref["t"])[1:], "points": ref["X"]}, spread, ("poses", "points"))


@pytest.mark.parametrize("name", list(lc.STRUCTURAL))
def test_rig_structural_failures_stop_the_loop_and_return_the_start(ctx, name):
    """A camera without observations (camera 5 of 6; camera 31 of the 32 x 64 problem, where D = 186 and the factor lives in
    global memory): its block of S is exactly 0 and the pivot test fails on any hardware, at any damping.  From lambda0 = 1e-3:
    two iterations, the Cholesky stop, rows (cost0, 1e-3, 0, 0) and (cost0, 2e-3, 0, 0).  From 6e15 or 1e16: one iteration, the
    lambda stop.  Exactly so, and poses and points come back as they went in, bit for bit.
    Measured on the MI355X: all five as stated; the start cost differs from the restatement's by 0 (its spread: 0 for the six
    cameras, 1.1e-16 for the 32)."""
    c = lc.rig_case(name)
    base, same, spread = lc.rig_reference(name)
    assert same
    got = rig_run(ctx, name)
    walk(name, got["history"], got["status"], got["iterations"], got["cost_initial"], base, spread)
    lambda0 = c["kw"]["lambda0"]
    rows = 1 if lambda0 >= 6e15 else 2
    assert got["status"] == (rb.STOP_LAMBDA if rows == 1 else rb.STOP_CHOLESKY) and got["iterations"] == rows
    assert got["history"].tolist() == [[got["cost_initial"], lambda0 * 2.0 ** i, 0.0, 0.0] for i in range(rows)]
    assert got["cost"] == got["cost_initial"]
    R, t, X = c["start"]
    assert got["poses"][1:].tobytes() == poses12(R, t)[1:].tobytes() and got["points"].tobytes() == np.ascontiguousarray(X).tobytes()
    assert got["poses"][0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


# ---- the intrinsics ---------------------------------------------------------------------------------------------------------------
def layout(cams):
    """(view_offset, point_offset, obj_xy, img_uv, image_sizes) of a list of ir.Camera"""
    voff, poff, obj, img = [0], [0], [], []
    for cam in cams:
        for o, u in cam.views:
            obj.append(o), img.append(u)
            poff.append(poff[-1] + len(o))
        voff.append(voff[-1] + len(cam.views))
    return voff, poff, np.concatenate(obj), np.concatenate(img), [cam.size for cam in cams]


def intr_run(ctx, cams, starts, **kw):
    """ctx.intrinsics_calibrate on a list of cameras from their starts (kd, R, t); per camera a dict of its share of every
    output, as bytes-comparable arrays"""
    start = (np.array([s[0] for s in starts]), np.concatenate([poses12(s[1], s[2]) for s in starts]))
    out = ctx.intrinsics_calibrate(*layout(cams), start, **kw)
    voff = np.cumsum([0] + [len(cam.views) for cam in cams])
    return [{"kd": out["kd"][c], "poses": out["poses"][voff[c]:voff[c + 1]], "view_rms": out["view_rms"][voff[c]:voff[c + 1]],
             "history": out["history"][c], "status": int(out["status"][c]), "iterations": int(out["iterations"][c]),
             "cost_initial": float(out["cost_initial"][c]), "cost": float(out["cost"][c])} for c in range(len(cams))]


def same_bytes(a, b):
    for k in ("kd", "poses", "view_rms", "history"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert all(a[k] == b[k] for k in ("status", "iterations", "cost_initial", "cost"))


def intr_walk(name, got, cam, base, spread):
    walk(name, got["history"], got["status"], got["iterations"], got["cost_initial"], base, spread)
    assert got["cost"] == got["history"][-1, 0]
    n = np.array([len(o) for o, _ in cam.views])
    assert abs(np.sum(n * got["view_rms"] ** 2) / (2 * got["cost"]) - 1) <= 1e-12  # view_rms is of the buffer handed back
    state_difference(name, got, {"kd": base["kd"], "poses": poses12(base["R"], base["t"])}, spread, ("kd", "poses"))


@pytest.mark.parametrize("name", list(lc.INTR))
def test_intrinsics_loop_walks_the_restatement_through_rejections(ctx, name):
    """lm_cases.INTR, one camera per call, the start handed in: rejections by the gain ratio in the middle of a run (mild_rho,
    golden_rho), nine leading rejections for a point behind the camera although rho = 0.91 (golden_behind), and the same run cut
    by max_iters = 6 while still rejecting, so that the start comes back (golden_behind_cut).  As the rig walk; also the
    returned kd and poses within 8 x the restatement's spread, and sum n_v view_rms_v^2 = 2 cost.
    Restatement's spread (CPU), cost / lambda / |step| / kd / poses        GPU - restatement (MI355X)
      mild_rho           8.4e-13 / 3.6e-10 / 4.0e-09 / 2.6e-15 / 3.1e-15     2.2e-16 / 1.1e-15 / 0 / 0 / 0   (21 iterations, ftol)
      golden_rho         1.2e-09 / 3.7e-09 / 1.2e-08 / 1.9e-15 / 2.6e-15     8.0e-10 / 2.6e-09 / 5.0e-09 / 1.0e-15 / 1.9e-15   (12, ftol)
      golden_behind      4.4e-16 / 0 / 7.5e-08 / 5.9e-16 / 2.9e-17           2.2e-16 / 0 / 0 / 0 / 0   (16, max_iters)
      golden_behind_cut  2.2e-16 / 0 / 7.5e-08 / 0 / 0                       1.1e-16 / 0 / 0 / 0 / 0   (6, max_iters)"""
    c = lc.intr_case(name)
    base, same, spread = lc.intr_reference(name)
    assert same
    got = intr_run(ctx, [c["cam"]], [c["start"]], **c["kw"])[0]
    intr_walk(name, got, c["cam"], base, spread)
    if name == "golden_behind_cut":
        kd, R, t = c["start"]
        assert got["kd"].tobytes() == kd.tobytes() and got["poses"].tobytes() == poses12(R, t).tobytes()


def test_intrinsics_state_after_trailing_rejections_is_the_last_accepted_one(ctx):
    """mild_rho cut at max_iters = 3, after its third accepted step, and at 6, after the three rejected steps that follow: the
    same bits of kd, poses, view_rms and cost (view_rms comes from the buffer the state record points at, not the trial's).
    The run cut at 6 against the restatement: spread (CPU) cost 8.4e-13, |step| 2.7e-12, kd 2.6e-14, poses 5.3e-14; GPU -
    restatement (MI355X) cost 2.2e-16, the rest 0."""
    c = lc.intr_case("mild_rho")
    k, j = lc.trailing_rejections(lc.intr_reference("mild_rho")[0])
    assert (k, j) == (3, 3)
    short = intr_run(ctx, [c["cam"]], [c["start"]], **dict(c["kw"], max_iters=k))[0]
    long = intr_run(ctx, [c["cam"]], [c["start"]], **dict(c["kw"], max_iters=k + j))[0]
    ref, same, spread = lc.intr_reference("mild_rho", k + j)
    assert same and lc.sequence(ref) == "1" * k + "0" * j
    assert short["status"] == long["status"] == ir.STOP_MAX_ITERS and (short["iterations"], long["iterations"]) == (k, k + j)
    for key in ("kd", "poses", "view_rms"):
        assert short[key].tobytes() == long[key].tobytes(), key
    assert short["cost"] == long["cost"] and long["history"][:k].tobytes() == short["history"].tobytes()
    intr_walk("mild_rho cut at 6", long, c["cam"], ref, spread)


def test_three_cameras_of_one_call_reject_and_stop_each_on_its_own(ctx):
    """lm_cases.TRIO in one call (lambda0 = 1e-3, max_iters = 22): mild_rho rejects three steps by rho in the middle and stops on
    ftol after 21 iterations, golden_behind starts with seven rejections for a point behind and one by rho and runs into
    max_iters at 22, golden_rho accepts every step and stops on ftol after 12: in iteration 0 one camera accepts while another
    rejects, and the launches go on for two cameras after the third has stopped.  Each camera's history and state against its
    own restatement as in the walk above, and each camera's outputs in bits those of a call with that camera alone.
    Restatement's spread (CPU), cost / lambda / |step| / kd / poses        GPU - restatement (MI355X)
      mild_rho       8.4e-13 / 3.6e-10 / 4.0e-09 / 2.6e-15 / 3.1e-15     2.2e-16 / 1.1e-15 / 0 / 0 / 0
      golden_behind  4.4e-16 / 0 / 4.1e-11 / 1.1e-15 / 1.1e-11           2.2e-16 / 0 / 0 / 0 / 3.1e-14
      golden_rho     5.9e-12 / 1.6e-09 / 1.1e-08 / 2.4e-15 / 3.2e-15     2.3e-12 / 1.1e-09 / 3.3e-09 / 6.2e-16 / 1.4e-15"""
    cases = [lc.intr_case(n) for n in lc.TRIO]
    kw = {"max_iters": lc.TRIO_MAX_ITERS, "ftol": ir.LOOP_FTOL, "lambda0": lc.TRIO_LAMBDA0}
    together = intr_run(ctx, [c["cam"] for c in cases], [c["start"] for c in cases], **kw)
    refs = [lc.trio_reference(n) for n in lc.TRIO]
    assert len({r[0]["iterations"] for r in refs}) == 3
    for name, c, got, (base, same, spread) in zip(lc.TRIO, cases, together, refs):
        assert same
        intr_walk("trio " + name, got, c["cam"], base, spread)
        same_bytes(got, intr_run(ctx, [c["cam"]], [c["start"]], **kw)[0])
    assert (together[0]["history"][0, 2], together[1]["history"][0, 2]) == (1.0, 0.0)


def test_intrinsics_structural_failure_stops_one_camera_and_not_its_neighbour(ctx):
    """lm_cases.singular_camera beside mild_rho in one call: the view without extent fails the 6x6 factorisation at every
    damping, so its camera stops after two iterations on the Cholesky stop (lambda0 = 1e-3) or after one on lambda (6e15) with
    the rows (cost0, lambda0 2^i, 0, 0) and its start handed back in bits, while its neighbour gives the bits it gives alone."""
    s, c = lc.singular_camera(), lc.intr_case("mild_rho")
    kd, R, t = s["start"]
    for lambda0, status, rows in ((1e-3, ir.STOP_CHOLESKY, 2), (6e15, ir.STOP_LAMBDA, 1)):
        kw = {"max_iters": 10, "ftol": ir.LOOP_FTOL, "lambda0": lambda0}
        ref = ir.lm(s["cam"], kd, R, t, **kw)
        got, beside = intr_run(ctx, [s["cam"], c["cam"]], [s["start"], c["start"]], **kw)
        assert ref["status"] == status and ref["iterations"] == rows
        assert got["status"] == status and got["iterations"] == rows
        assert got["history"].tolist() == [[got["cost_initial"], lambda0 * 2.0 ** i, 0.0, 0.0] for i in range(rows)]
        assert abs(got["cost_initial"] / ref["cost_initial"] - 1) < 1e-12 and got["cost"] == got["cost_initial"]
        assert got["kd"].tobytes() == kd.tobytes() and got["poses"].tobytes() == poses12(R, t).tobytes()
        assert np.abs(got["view_rms"] / ref["view_rms"] - 1).max() <= 1e-12
        same_bytes(beside, intr_run(ctx, [c["cam"]], [c["start"]], **kw)[0])
