"""The residual problems of tests/ba_cases.py on the CPU: what test_gpu_geom's tests beyond 256 groups rely on, from the oracle
(oracle/geom_oracle.c: orc_ba_residuals, the reference's lib/Helpers.py:161-167) and from the reference's rule written out."""
import numpy as np

import ba_cases as bc
import oracle


def test_the_holes_put_every_later_group_below_its_index():
    valid = bc.holes()
    assert valid.shape == (600, 3) and int((valid == 0).sum()) == len(bc.ONE_VIEW_MISSING) + 3 + 2
    full = valid.all(axis=1)
    obj_index = np.cumsum(full) - 1  # of the groups that are triangulated
    assert (obj_index[:3] == np.arange(3)).all() and (obj_index[256:][full[256:]] < np.arange(256, 600)[full[256:]]).all()
    # both loops cross the round boundaries out of step: the first round leaves 253 object points, the first two 504
    assert int(full[:256].sum()) == 253 and int(full[:512].sum()) == 504
    nobj, nres = bc.lengths_by_the_rule(valid)
    assert (nobj, nres) == (bc.N_TRIANGULATED, bc.N_RESIDUALS) == (591, 589)
    # the pairs the second loop drops: one in its first round, one in its second
    assert [n for n in range(nobj) if valid[n].sum() <= 1] == [bc.UNSEEN, bc.ONE_CAMERA] and bc.UNSEEN < 256 <= bc.ONE_CAMERA < 512
    assert bc.lengths_by_the_rule(np.ones((600, 3))) == (600, 600)


def test_the_oracle_follows_the_rule_and_solves_every_group_of_a_hole_free_problem_on_its_own():
    """With the holes the oracle gives 591 object points and 589 of 600 residuals (about 1 s); without holes, the residuals of
    groups 0..255 and 256..511 alone are rows [0, 256) and [256, 512) of the 600-group answer, to the bit"""
    p = bc.problem(600)
    valid = bc.holes()
    for x in p["sets"][:2]:
        e = oracle.ba_residuals(x, bc.C, p["pts"], valid, p["K"], p["dist"])
        assert e.dtype == np.float32 and len(e) == bc.N_RESIDUALS and np.isfinite(e).all()
        whole = oracle.ba_residuals(x, bc.C, p["pts"], np.ones((600, 3), np.uint8), p["K"], p["dist"])
        assert len(whole) == 600
        for lo in (0, 256):
            part = oracle.ba_residuals(x, bc.C, p["pts"][lo:lo + 256], np.ones((256, 3), np.uint8), p["K"], p["dist"])
            assert part.tobytes() == whole[lo:lo + 256].tobytes()
    # the positional pairing shows: from the first hole on, the residuals are those of mismatched pairs
    assert not np.allclose(e[4:200], whole[4:200], rtol=1e-3)
