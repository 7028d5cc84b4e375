"""CPU: the planted two-camera SearchByProjection cases (tests/sbp_two_patterns.py) through the definition
(oracle/sbp_definition.py, py_sbp_local_two / py_sbp_lastframe_two) and the C++ oracle's two-camera entries. For
every case: the definition's slots and return value equal the hand-derived expectation, at every th the case
allows; the oracle equals it; the case's own trace assertion holds (the rule it names decided); every wrong
reading the case names (`variant=`) answers differently; and padding to 2,049 keypoints or 2,049 points changes no
planted slot and no count and leaves every appended slot at -1. Every variant of the definition must be told apart
by at least one case. No case is skipped."""
import numpy as np
import pytest

import sbp_two_patterns as P
from oracle import sbp_definition as sd

CASES = P.all_cases()
VARIANTS = {"local2": sd.LOCAL_TWO_VARIANTS + sd.LOCAL_TWO_EXTRA,
            "lastframe2": sd.LASTFRAME_TWO_VARIANTS + sd.LASTFRAME_TWO_EXTRA}


def test_every_variant_has_a_case():
    for kind, names in VARIANTS.items():
        killed = {v for c in CASES if c.kind == kind for v in c.variant}
        assert killed <= set(names), killed - set(names)
        for v in names:
            assert v in killed, f"no {kind} case tells '{v}' from the reference"
    assert all(c.variant for c in CASES)


def test_case_inventory():
    names = {c.name for c in CASES}
    for need in ("four-writes", "link-guards", "partner-overwrites", "last-writer-2", "last-writer-6", "last-writer-7",
                 "own-partner-seen", "left-ratio-cancels-right", "left-far-right-runs", "gates", "right-radius",
                 "right-window-edge", "right-ties-ratio", "list-depth-4", "list-depth-5", "ladder", "ladder-reversed",
                 "cameras-apart"):
        assert need + "-local2" in names, need
    for need in ("two-entries", "left-window", "right-outside", "right-claims", "ladder-obs1", "ladder-obs0", "list-overflow",
                 "preheld", "no-uright-gate", "gates", "level-range-L0-std", "level-range-L7-fw", "level-range-L0-fw",
                 "level-range-L7-bw", "rot-ties-ori1", "rot-tenth-60-ori1", "rot-half-way-ori1", "rot-ties-ori0"):
        assert need + "-lastframe2" in names, need
    assert P.SEVEN_WRITERS in names
    assert {th for c in CASES if c.kind == "local2" for th in c.ths} == {1, 3}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(oracle_lib, case):
    for th in case.ths:
        c = case if th == case.par["th"] else P.with_th(case, th)
        n_d, tr, mvp_d = P.run_definition(c)
        n_o, mvp_o = P.run_oracle(oracle_lib, c)
        assert n_d == case.n and n_o == case.n, (th, n_d, n_o, case.n)
        np.testing.assert_array_equal(mvp_d, case.expect, err_msg=f"definition, th {th}")
        np.testing.assert_array_equal(mvp_o, case.expect, err_msg=f"oracle, th {th}")
        case.check(c, tr)
    for v in case.variant:
        n_v, _, mvp_v = P.run_definition(case, v)
        assert n_v != case.n or (mvp_v != case.expect).any(), f"'{v}' no longer answers differently"
    for padded in (P.pad_keys(case), P.pad_queries(case)):
        assert (padded.F.N == P.PAD_N) != (len(padded.q) == P.PAD_N)
        assert padded.F.nleft == case.F.nleft and (padded.F.l2r == case.F.l2r).all()
        n_p, tr_p, mvp_p = P.run_definition(padded)
        n_po, mvp_po = P.run_oracle(oracle_lib, padded)
        assert n_p == n_po == case.n
        np.testing.assert_array_equal(mvp_po, mvp_p)
        np.testing.assert_array_equal(mvp_p[:case.F.N], case.expect)
        assert (mvp_p[case.F.N:] == -1).all()
        case.check(padded, tr_p)
