"""GPU parity of the two-camera SearchByProjection forms (Frame.Nleft != -1) on the planted cases of
tests/sbp_two_patterns.py (each proved on the CPU to reach the rule it names, tests/test_sbp_two_definition.py):
every case through every form its kind has, every slot and the return value equal to the C++ oracle's and to the
hand-derived expectation.

Which form runs is decided by sbp_run (orbfe_matcher.hip) from the shape alone:
  local map, n <= 2048 and nq <= 2048        k_sbp_block4 (9), one workgroup                       as planted
  the same, a slot with 7 writers in a pass  k_sbp_block4 aborts -> k_sbp_local2 (11)              last-writer-7
  local map, n > 2048 or nq > 2048           k_sbp_local2 + k_slot_count / _scan / _fill (11)      keys / points padded
  last frame, n <= 2048 and nq <= 2048       k_sbp_block2 (10), one workgroup                      as planted
  last frame, n > 2048 or nq > 2048          k_sbp_proj2 (12)                                      keys / points padded
Padding goes to 2,049, one past the limits, and is inert (sbp_two_patterns.pad_keys / pad_queries). Every run
asserts the form the driver recorded (orbfe_matcher_last_form), so a moved threshold fails here instead of quietly
testing another kernel. Each shape runs twice on one ORBmatcher with a different case in between (stale arena or
per-thread state would show in the second run). Local-map cases run at every th they allow (th scales the left
radius only)."""
import numpy as np
import pytest

import sbp_two_patterns as P
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.matcher import ORBmatcher

pytestmark = pytest.mark.gpu

CASES = P.all_cases()
# orbfe_matcher_last_form (include/orbfe.h)
FORM_BLOCK4, FORM_BLOCK2, FORM_LOCAL2, FORM_PROJ2 = 9, 10, 11, 12


def _run_gpu(m, c):
    mvp, p = c.mvp0.copy(), c.par
    m.mfNNratio, m.mbCheckOrientation = float(p["nnratio"]), bool(p["check_ori"])
    if c.kind == "local2":
        n = m.SearchByProjectionLocalMap(c.F, mvp, c.obs, c.q, p["th"], p["bfar"], p["thfar"])
    else:
        n = m.SearchByProjectionLastFrameStereo(c.F, mvp, c.obs, c.q, c.ruv, p["th"], p["fw"], p["bw"])
    return n, mvp, _lib.load().orbfe_matcher_last_form()


def _form(case, padded):
    if case.kind == "local2":
        return FORM_LOCAL2 if padded or case.name == P.SEVEN_WRITERS else FORM_BLOCK4
    return FORM_PROJ2 if padded else FORM_BLOCK2


def _other(case):
    """A different case of the other kind where one exists (another kernel runs in between)."""
    i = CASES.index(case)
    return next(c for c in CASES[i + 1:] + CASES[:i] if c.kind != case.kind)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_every_form(gpu, oracle_lib, case):
    m = ORBmatcher()
    between = _other(case)
    forms = []
    for th in case.ths:
        c_th = case if th == case.par["th"] else P.with_th(case, th)
        n_o, mvp_o = P.run_oracle(oracle_lib, c_th)
        assert n_o == case.n
        np.testing.assert_array_equal(mvp_o, case.expect)
        for padded in (None, "queries", "keys"):
            c = c_th if padded is None else P.pad_queries(c_th) if padded == "queries" else P.pad_keys(c_th)
            assert (c.F.N > 2048) == (padded == "keys") and (len(c.q) > 2048) == (padded == "queries")
            want = _form(case, padded)
            for rep in range(2):
                n, mvp, form = _run_gpu(m, c)
                print(f"{c.name} th {th} run {rep}: form {form} nmatches {n}")
                assert form == want, (c.name, th, rep, form, want)
                assert n == n_o, (c.name, th, rep, form, n, n_o)
                np.testing.assert_array_equal(mvp[:case.F.N], mvp_o, err_msg=f"{c.name} th {th} run {rep} form {form}")
                assert (mvp[case.F.N:] == -1).all(), (c.name, form)
                if rep == 0:
                    nb, mb, _ = _run_gpu(m, between)
                    assert nb == between.n
                    np.testing.assert_array_equal(mb, between.expect)
            forms.append(want)
    assert set(forms) == ({FORM_BLOCK4, FORM_LOCAL2} if case.kind == "local2" and case.name != P.SEVEN_WRITERS else
                          {FORM_LOCAL2} if case.kind == "local2" else {FORM_BLOCK2, FORM_PROJ2})


def test_seven_writers_arrive_at_the_multi_launch_form(gpu, oracle_lib):
    """6 writers of one slot stay in k_sbp_block4; the 7th makes it abort with nothing written, and the call
    reports the multi-launch form with the same slots."""
    by = {c.name: c for c in CASES}
    six, seven = by["last-writer-6-local2"], by[P.SEVEN_WRITERS]
    m = ORBmatcher()
    for c, want in ((six, FORM_BLOCK4), (seven, FORM_LOCAL2), (six, FORM_BLOCK4)):
        n, mvp, form = _run_gpu(m, c)
        print(f"{c.name}: form {form} nmatches {n}")
        assert form == want and n == c.n
        np.testing.assert_array_equal(mvp, c.expect)
