"""CPU: the planted SearchByProjection cases (tests/sbp_patterns.py) through the definition
(oracle/sbp_definition.py) and the C++ oracle. For every case, plain and padded to 2,049 keypoints or
2,049 queries: the oracle's slots and return value equal the definition's; the definition's trace shows
that the rule the case names decided (the case's own `check`); padding changes no planted slot and no
count; and where the rule is float-sensitive the double evaluation of it gives another answer, so a case
that stopped telling the two apart fails here. No case is skipped."""
import numpy as np
import pytest

import sbp_patterns as P
from oracle import sbp_definition as sd
from test_oracle_matcher import py_search_for_init

CASES = P.all_cases()
f32 = np.float32


def test_float_facts():
    """The three float facts the planted cases stand on."""
    for m in range(10, 121, 10):
        keep = sd.three_maxima_inds([m, m // 10] + [0] * 28)
        assert keep[1] == 1 and sd.three_maxima_inds([m, m // 10] + [0] * 28, double=True)[1] == -1
    assert not sd.ratio_rejects(63, 90, 0.7) and sd.ratio_rejects(63, 90, 0.7, double=True)
    assert not sd.ratio_rejects(75, 100, 0.75) and not sd.ratio_rejects(80, 100, 0.8)
    for a in P.HALF:
        rot = P.down(a)
        assert f32(rot * f32(f32(1) / f32(30))) == f32(a // 30 + 0.5) and float(rot) / 30.0 < a // 30 + 0.5
        assert sd.py_rot_bin(rot, 0.0) == a // 30 + 1 and sd.py_rot_bin(rot, 0.0, double=True) == a // 30


def test_case_inventory():
    names = {c.name.split("-th")[0].rsplit("-", 1)[0] for c in CASES}
    for need in ("window-edge", "window-cells", "window-offset-bounds", "level-range-L0-std", "level-range-L7-fw",
                 "level-range-L0-fw", "level-range-L7-bw", "tie-levels", "tie-dup-zero", "distance-100", "distance-80",
                 "ratio-0.6", "ratio-0.7", "ratio-0.75", "ratio-0.8", "ratio-0.9", "stereo-edge", "stereo-fused",
                 "ladder-obs1", "ladder-obs0", "list-overflow", "preheld-obs0", "rot-half-way-ori1", "rot-tenth-60-ori1"):
        assert need in names, need
    for kind, ths in (("local", {1, 3, 5}), ("lastframe", {1, 7}), ("kf", {1, 10})):
        assert {c.par["th"] for c in CASES if c.kind == kind} == ths


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(oracle_lib, case):
    n_d, tr, mvp_d = P.run_definition(case)
    n_o, mvp_o = P.run_oracle(oracle_lib, case)
    assert n_o == n_d
    np.testing.assert_array_equal(mvp_o, mvp_d)
    case.check(case, tr, mvp_d, n_d)
    if case.double is not None:
        diff = case.double(case)
        assert diff and all(diff), "the double evaluation no longer differs"
    for padded in (P.pad_keys(case), P.pad_queries(case)):
        assert padded.F.N == P.PAD_N or len(padded.q) == P.PAD_N
        n_p, tr_p, mvp_p = P.run_definition(padded)
        n_po, mvp_po = P.run_oracle(oracle_lib, padded)
        assert n_p == n_po == n_d
        np.testing.assert_array_equal(mvp_po, mvp_p)
        np.testing.assert_array_equal(mvp_p[:case.F.N], mvp_d)
        assert (mvp_p[case.F.N:] == -1).all()
        case.check(padded, tr_p, mvp_p, n_p)


@pytest.mark.parametrize("case", P.init_cases(), ids=repr)
def test_init_case(oracle_lib, case):
    """The bin plans through SearchForInitialization: oracle == py_search_for_init == the plan."""
    pa, pb = case.prev(), case.prev()
    ma = np.zeros(case.F1.N, np.int32)
    na = oracle_lib.OracleMatcher(0.9, True).search_for_init(case.F1, case.F2, pa, ma, 10)
    nb, mb = py_search_for_init(case.F1, case.F2, pb, 0.9, 10, True)
    assert na == nb == int((case.expect >= 0).sum())
    np.testing.assert_array_equal(ma, mb)
    np.testing.assert_array_equal(ma, case.expect)
