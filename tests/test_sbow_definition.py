"""CPU: the planted SearchByBoW cases (tests/sbow_patterns.py) through the definition
(oracle/sbow_definition.py) and the C++ oracle. For every case, plain, with the frame side padded and with
the keyframe side padded past the one-workgroup bounds: the oracle's slots and return value equal the
definition's; the definition's trace shows that the rule the case names decided (the case's own `check`);
padding changes no planted slot and no count and its own slots stay -1; and where the rule is
float-sensitive the double evaluation gives other slots, so a case that stopped telling the two apart
fails here. No case is skipped."""
import numpy as np
import pytest

import sbow_patterns as P
from oracle import sbow_definition as bd
from oracle import sbp_definition as sd

CASES = P.all_cases()
f32 = np.float32


def test_float_facts():
    """The float facts the planted cases stand on."""
    for d1, d2 in P.FLOAT_PAIRS:   # the product in float lies above d1, the double product does not
        assert f32(d1) < f32(f32(0.6) * f32(d2)) and not d1 < 0.6 * d2
        assert bd.ratio_passes(d1, d2, 0.6) and not bd.ratio_passes(d1, d2, 0.6, double=True)
    for r in P.RATIOS:   # no other pair with d1 <= 50 tells float from double, at any of the five ratios
        diff = {(a, b) for b in range(1, 257) for a in range(0, 51)
                if bd.ratio_passes(a, b, r) != bd.ratio_passes(a, b, r, double=True)}
        assert diff == (set(P.FLOAT_PAIRS) if r == 0.6 else set()), (r, diff)
        d1, d2 = P.EQ_PAIR[r]
        assert f32(d1) == f32(f32(r) * f32(d2)) and not bd.ratio_passes(d1, d2, r)
        assert bd.ratio_passes(d1 - 1, d2, r) and not bd.ratio_passes(d1 + 1, d2, r)
    assert sd.py_rot_bin(P.f32(900.0), 0.0) == 0   # round(rot / 30) == 30 wraps to bin 0


def test_case_inventory():
    names = {c.name for c in CASES}
    need = ["distance-50", "distance-51", "ratio-0.6-float", "best-tie-rejected", "mp-skip", "empty-node", "join",
            "unlisted", "right-inside-left", "right-needs-left", "right-ignores-ratio", "right-tie", "nleft-edge",
            "nleft-edge-0", "nleft-edge-n", "rot-two-entries", "kk-distance-49", "kk-distance-50", "kk-ratio-0.6-float",
            "kk-mp2-skip", "kk-mp-skip", "kk-right-skipped-1", "kk-right-skipped-2", "kk-best-tie-rejected", "kk-join"]
    need += [f"{k}ratio-{r}" for k in ("", "kk-") for r in P.RATIOS] + [f"lone-candidate-{r}" for r in P.RATIOS]
    need += ["distance-50-wide", "distance-51-wide", "ratio-0.6-float-wide", "right-inside-left-wide"]
    need += [f"ratio-{r}-wide" for r in P.RATIOS]
    need += [f"{k}ladder-{m}" for k in ("", "kk-") for m in (6, 17, 35)]
    need += [f"node-size-{m}" for m in (1, 3, 4, 5, 16, 17, 33)]
    need += [f"{k}rot-{p}-ori{o}" for k in ("", "kk-") for p in P.PLANS for o in (0, 1)]
    for n in need:
        assert n in names, n
    assert {"half-way", "tenth-10", "ties", "angles", "zero-bins"} <= set(P.PLANS)
    join = next(c for c in CASES if c.name == "join")
    assert len(set(join.a.fv.node_ids.tolist()) & set(join.b.fv.node_ids.tolist())) > 256
    # the padded shapes cross the drivers' bounds, the planted ones do not
    for c in CASES:
        da, db, npairs = P.dims(c.a), P.dims(c.b), P._npairs(c)
        assert P.fits_block(da, db, npairs) and P.fits_batch(da, db) and c.a.N <= 400 and c.b.N <= 400, c.name
    c = CASES[0]
    kf, fr = P.pad_keyframe(c), P.pad_frame(c)
    assert not P.fits_block(P.dims(kf.a), P.dims(c.b), P._npairs(c)) and not P.fits_batch(P.dims(kf.a), P.dims(c.b))
    assert not P.fits_block(P.dims(c.a), P.dims(fr.b), P._npairs(c))
    assert kf.a.N <= 4200 and fr.b.N <= 4200   # no larger than the shapes the random-frame tests use


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(oracle_lib, case):
    n_d, s_d, tr = P.run_definition(case)
    n_o, s_o = P.run_oracle(oracle_lib, case)
    assert n_o == n_d == int((s_d >= 0).sum())
    np.testing.assert_array_equal(s_o, s_d)
    case.check(case, tr, s_d, n_d)
    if case.sens:
        _, s_x, _ = P.run_definition(case, double=True)
        assert not np.array_equal(s_x, s_d), "the double evaluation no longer differs"
    for padded in (P.pad_frame(case), P.pad_keyframe(case)):
        n_p, s_p, tr_p = P.run_definition(padded)
        n_po, s_po = P.run_oracle(oracle_lib, padded)
        assert n_p == n_po == n_d
        np.testing.assert_array_equal(s_po, s_p)
        np.testing.assert_array_equal(s_p[:len(s_d)], s_d)
        assert (s_p[len(s_d):] == -1).all()
        assert tr_p["nodes"] == tr["nodes"]
        case.check(padded, tr_p, s_p, n_p)
