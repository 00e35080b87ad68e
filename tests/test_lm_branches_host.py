"""What tests/test_gpu_lm_branches.py stands on, established on the restatements alone (tests/lm_ref.py's control through
tests/rig_ba_ref.py, tests/rig_robust_ref.py and tests/intrinsics_ref.py): every case of tests/lm_cases.py takes the branches
it is there for, and is far enough from each of its decision boundaries that the order of the sums (all that the kernels do
differently) cannot change a decision.  Every margin and spread asserted here is printed."""
import numpy as np
import pytest

import intrinsics_ref as ir
import lm_cases as lc
import rig_ba_ref as rb

RIG_NAMES = list(lc.RIG) + list(lc.STRUCTURAL)
# what the named cases were chosen for: the accept sequence and the stop
EXPECTED = {
    "A": ("10001111111111", rb.STOP_FTOL), "B": ("1100000111111111", rb.STOP_FTOL), "C": ("11000011000", rb.STOP_MAX_ITERS),
    "D": ("00", rb.STOP_CHOLESKY), "F": ("0000011111110011111111111", rb.STOP_FTOL), "G9": ("0010011111111111", rb.STOP_FTOL),
    "G22": ("11000011111111111111", rb.STOP_FTOL), "E_chol": ("00", rb.STOP_CHOLESKY), "E_lambda": ("0", rb.STOP_LAMBDA),
    "E_lambda_1e16": ("0", rb.STOP_LAMBDA), "E32_chol": ("00", rb.STOP_CHOLESKY), "E32_lambda": ("0", rb.STOP_LAMBDA),
    "mild_rho": ("111000111111111111111", rb.STOP_FTOL), "golden_rho": ("111000011111", rb.STOP_FTOL),
}


def margins(name, base, ftol, depth_margin, pivot_of):
    """Asserts the margins of one restatement run, printing each; depth_margin(trial state), pivot_of(trace entry) -> (pivot,
    largest diagonal) or None"""
    acc, rho, h = base["history"][:, 2] > 0, base["rho"], base["history"]
    solved = ~np.isnan(rho)
    print(f"{name}: accepted {lc.sequence(base)}  status {base['status']}  iterations {base['iterations']}")
    print(f"{name}: rho {rho}")
    assert (np.abs(rho[solved]) >= 1e-3).all(), (name, rho)
    for it in np.flatnonzero(~acc & solved & (np.nan_to_num(rho) > 0)):  # rejected although the cost went down: a point behind
        d = depth_margin(base["trace"][it]["trial"])
        print(f"{name}: iteration {it} rejected for a point behind: rho {rho[it]:.4f}, most negative depth {d:.3e} of the point's distance")
        assert rho[it] > 1e-3 and d < -1e-6, (name, it)
    for it in np.flatnonzero(~solved):
        piv = pivot_of(base["trace"][it])
        assert piv is not None, (name, it)
        print(f"{name}: iteration {it} failed solve: pivot {piv[0]:.4e}, largest diagonal entry {piv[1]:.4e}")
        assert piv[0] == 0.0 or piv[0] <= -1e-6 * piv[1], (name, it)
    prev = np.r_[base["cost_initial"], h[:-1, 0]]
    rel = (prev - h[:, 0])[acc] / prev[acc]
    print(f"{name}: relative decrease of the accepted steps / ftol {rel / ftol}")
    assert not ((rel > ftol / 1.2) & (rel < ftol * 1.2)).any(), (name, rel)
    # the stop on lambda: no damping within a factor 1.2 of 1e16 after a rejection
    after = h[~acc, 1] * 2.0 ** np.arange(1, 64)[_run_lengths(acc)]
    assert not ((after > 1e16 / 1.2) & (after < 1e16 * 1.2)).any(), (name, after)


def _run_lengths(acc):
    """for every rejected iteration, its position (from 0) in its run of rejections"""
    out, j = [], 0
    for a in acc:
        j = 0 if a else j + 1
        if not a:
            out.append(j - 1)
    return np.array(out, int)


def show_spread(name, same, spread):
    print(f"{name}: same decisions under {lc.N_PERM} permutations {same}; spread " +
          "  ".join(f"{k} {float(np.max(v)) if np.size(v) else 0.0:.3e}" for k, v in spread.items()))
    for k in ("cost", "lambda", "step"):
        print(f"{name}: {k} spread per iteration {spread[k]}")


def rig_pivot(entry):
    return lc.failing_pivot(entry["S"])


def intr_pivot(entry):
    """the first failing factor of an intrinsics iteration: a view's V*, else S"""
    lin = entry["lin"]
    for v, L in enumerate(lin["L"]):
        if L is None:
            Vd = lin["V"][v].copy()
            Vd[np.diag_indices(6)] = np.diag(Vd) + entry["lam"] * np.diag(Vd)
            return lc.failing_pivot(Vd)
    return lc.failing_pivot(lin["S"])


@pytest.mark.parametrize("name", RIG_NAMES)
def test_rig_case_is_far_from_every_decision_boundary(name):
    c = lc.rig_case(name)
    base, same, spread = lc.rig_reference(name)
    show_spread(name, same, spread)
    assert same
    if name in EXPECTED:
        assert (lc.sequence(base), base["status"]) == EXPECTED[name]
    margins(name, base, c["kw"]["ftol"], lambda state: lc.rig_depth_margin(c["prob"], state), rig_pivot)
    if name in lc.STRUCTURAL:  # the failure is structural: the camera's block of S is exactly 0, and the start comes back
        cams = c["prob"].C
        for entry in base["trace"]:
            assert not entry["S"][6 * (cams - 2):, :].any() and not entry["S"][:, 6 * (cams - 2):].any()
        cost0, lam0 = base["cost_initial"], c["kw"]["lambda0"]
        assert base["history"].tolist() == [[cost0, lam0 * 2.0 ** i, 0.0, 0.0] for i in range(base["iterations"])]
        R, t, X = c["start"]
        assert np.array_equal(base["t"][1:], t[1:]) and np.array_equal(base["R"][1:], R[1:]) and np.array_equal(base["X"], X)


@pytest.mark.parametrize("name", list(lc.INTR))
def test_intrinsics_case_is_far_from_every_decision_boundary(name):
    c = lc.intr_case(name)
    base, same, spread = lc.intr_reference(name)
    show_spread(name, same, spread)
    assert same
    if name in EXPECTED:
        assert (lc.sequence(base), base["status"]) == EXPECTED[name]
    margins(name, base, c["kw"]["ftol"], lambda state: lc.intr_depth_margin(c["cam"], state), intr_pivot)


def test_the_three_cameras_of_one_call_part_ways():
    """lc.TRIO under one lambda0 and max_iters: in some iteration one camera accepts while another rejects, the three stop at
    three different iterations, and each is far from its decision boundaries"""
    runs = {}
    for name in lc.TRIO:
        c = lc.intr_case(name)
        base, same, spread = lc.trio_reference(name)
        show_spread("trio " + name, same, spread)
        assert same
        margins("trio " + name, base, c["kw"]["ftol"], lambda state: lc.intr_depth_margin(c["cam"], state), intr_pivot)
        runs[name] = base
    first, second, third = (runs[n] for n in lc.TRIO)
    assert "rho-rejection" in lc.branches(first) and lc.sequence(first).startswith("1")
    assert lc.sequence(second).startswith("0") and second["rho"][0] > 1e-3  # begins with a rejection for a point behind
    assert set(lc.sequence(third)) == {"1"}
    assert len({r["iterations"] for r in runs.values()}) == 3
    both = min(first["iterations"], second["iterations"])
    assert (first["history"][:both, 2] != second["history"][:both, 2]).any()


def test_the_singular_view_fails_every_solve():
    """lc.singular_camera: the first pivot of view 2's V* is exactly 0, so every solve fails whatever the damping: two
    iterations and the Cholesky stop from lambda0 = 1e-3, one and the lambda stop from 6e15; the start comes back"""
    c = lc.singular_camera()
    kd, R, t = c["start"]
    for lambda0, status, rows in ((1e-3, ir.STOP_CHOLESKY, 2), (6e15, ir.STOP_LAMBDA, 1)):
        trace = []
        run = ir.lm(c["cam"], kd, R, t, ftol=ir.LOOP_FTOL, lambda0=lambda0, trace=trace)
        for entry in trace:
            piv = intr_pivot(entry)
            print(f"singular view, lambda0 {lambda0}: pivot {piv[0]}, largest diagonal entry {piv[1]:.4e}")
            assert entry["lin"]["L"][2] is None and piv[0] == 0.0 and not entry["lin"]["V"][2][:3].any()
        assert run["status"] == status and run["iterations"] == rows
        assert run["history"].tolist() == [[run["cost_initial"], lambda0 * 2.0 ** i, 0.0, 0.0] for i in range(rows)]
        assert np.array_equal(run["kd"], kd) and np.array_equal(run["R"], R) and np.array_equal(run["t"], t)


def test_the_table_covers_every_branch():
    """Each branch of lm_ref.control that the GPU tests are there for is taken by at least one case.
    Not in the table: a single failed solve followed by a solved step.  None was found that holds under permutation.  S of a
    Gauss-Newton step is positive semidefinite, so a pivot fails for rounding alone or for an exact zero that no damping
    cures: on case D's start, 40 values of lambda0 between 1e-8 and 4.6e-8 give failures followed by solved steps, and every
    such run decides differently under some permutation of the sums; so did the only find among 40 start seeds (seed 36,
    scale 0.8, lambda0 1e-8), whose first solve fails in the given order and succeeds in permuted ones.  Likewise no intrinsics
    start with a failing 6x6 or 9x9 factorisation of the margin was found: the failed solves of the intrinsics loop are the
    structural ones of lc.singular_camera."""
    rig = {name: lc.branches(lc.rig_reference(name)[0]) for name in RIG_NAMES}
    intr = {name: lc.branches(lc.intr_reference(name)[0]) for name in lc.INTR}
    for name, b in {**rig, **intr}.items():
        print(name, sorted(b))
    for branch in ("rho-rejection", "consecutive rejections", "accept after rejection", "trial_behind rejection",
                   "STOP_CHOLESKY", "STOP_LAMBDA", "STOP_MAX_ITERS on a rejection"):
        assert any(branch in b for b in rig.values()), ("rig", branch)
    for branch in ("rho-rejection", "trial_behind rejection", "STOP_MAX_ITERS on a rejection"):
        assert any(branch in b for b in intr.values()), ("intrinsics", branch)
    # the loss, two workgroups of points and the factor in global memory each meet a rejection or a failed solve
    assert "rho-rejection" in rig["F"] and lc.rig_case("F")["loss_c"] is not None
    assert lc.rig_case("G9")["prob"].N > 256 and "rho-rejection" in rig["G9"] and "trial_behind rejection" in rig["G22"]
    assert lc.rig_case("E32_chol")["prob"].D > 90 and "STOP_CHOLESKY" in rig["E32_chol"]


def test_trailing_rejections_are_where_the_gpu_test_cuts():
    """The returned-state test runs each loop to max_iters = k and to k + j, j rejections after the accepted iteration k - 1:
    the restatement hands back the same state from both"""
    for name, start, expect in (("A", 0, (1, 3)), ("F", 6, (12, 2)), ("G9", 0, (3, 2))):
        base = lc.rig_reference(name)[0]
        k, j = lc.trailing_rejections(base, start)
        assert (k, j) == expect, (name, k, j)
        a, b = lc.rig_reference(name, k)[0], lc.rig_reference(name, k + j)[0]
        assert lc.sequence(b) == lc.sequence(a) + "0" * j and a["status"] == b["status"] == rb.STOP_MAX_ITERS
        for key in ("R", "t", "X"):
            assert a[key].tobytes() == b[key].tobytes(), (name, key)
        assert a["cost"] == b["cost"]
    base = lc.intr_reference("mild_rho")[0]
    k, j = lc.trailing_rejections(base)
    assert (k, j) == (3, 3)
    a, b = lc.intr_reference("mild_rho", k)[0], lc.intr_reference("mild_rho", k + j)[0]
    for key in ("kd", "R", "t", "view_rms"):
        assert a[key].tobytes() == b[key].tobytes(), key
