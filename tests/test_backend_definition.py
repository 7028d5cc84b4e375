"""CPU: the planted back-end matcher cases (tests/backend_patterns.py) through the definition
(oracle/backend_definition.py) and the C++ oracle. For every case, plain and padded both ways (the
searched keyframe to 2,049 keypoints, the point list / the other keyframe to 2,049 records): the oracle's
return value and every output array equal the definition's; the definition's trace shows that the rule
the case names decided (the case's own `check`); padding changes no planted slot and no count; and every
careless evaluation the case lists (backend_definition's variants) gives another answer, so a case that
stopped telling the two apart fails here. No case is skipped."""
import numpy as np
import pytest

import backend_patterns as P
from oracle import backend_definition as bd

CASES = P.all_cases()
f32 = np.float32


def test_float_facts():
    """The float facts the planted cases stand on."""
    assert float(f32(7.8)) > 7.8 and float(P.down(f32(7.8))) < 7.8          # a product equal to 7.8f is rejected
    assert float(f32(5.99)) < 5.99 and float(P.up(f32(5.99))) > 5.99        # the nearest floats straddle 5.99
    assert float(f32(0.8)) > 0.8 and float(f32(1.2)) > 1.2 and float(f32(3.84)) != 3.84
    assert f32(f32(50) * f32(0.9)) == f32(45.0) and float(f32(50)) * float(f32(0.9)) < 45.0
    assert f32(f32(50) * f32(0.5)) == f32(25.0)
    assert not (f32(-0.0) < f32(0.0)) and f32(-1e-45) < f32(0.0) and f32(1e-45) > 0
    with np.errstate(all="ignore"):
        assert np.isinf(f32(256.0) * f32(1.0) / f32(1e-45)) and np.isinf(f32(1.0) / f32(0.0))
    assert P.SF[0] == 1.0 and f32(f32(P.TH) * P.SF[0]) == f32(4.0)
    for u in (0.0, 300.0, 751.0):                                           # depth 4: the three expressions agree
        pc = P.at_pixel(u, 100.0)
        got = {bd.project(e, f32(256), f32(256), f32(256), f32(256), pc)[:2] for e in
               (bd.PRJ_DIV, bd.PRJ_INVZ_F, bd.PRJ_INVZ_D)}
        assert got == {(f32(u), f32(100.0))}
    assert bd.sum3(f32(1e8), f32(-1e8), f32(1.0)) == 0.0 and bd.sum3(f32(1e8), f32(-1e8), f32(1.0), ("sum-order",)) == 1.0


def test_log_double_is_indistinguishable():
    """Why no scale-boundary case carries the "log-double" variant: within 200 floats of every level flip
    (ratio 1.2^k, k = -1..8) the rounded double log gives the level the float log gives."""
    for k in range(-1, 9):
        r = np.int32(f32(1.2 ** k).view(np.int32) - 200).view(np.float32)
        for _ in range(400):
            assert bd.raw_scale(r, f32(1.0), P.LOGSF) == bd.raw_scale(r, f32(1.0), P.LOGSF, ("log-double",)), (k, r)
            r = P.up(r)


def test_case_inventory():
    def family(c):
        return c.name[:-len(c.entry) - 1]
    names = {family(c) for c in CASES} | {f for c in CASES for f in c.covers}
    for need in P.REQUIRED:
        assert need in names, need
    by_entry = {}
    for c in CASES:
        by_entry.setdefault(c.entry, set()).update((family(c),) + tuple(c.covers))
    for e in P.PROJ_ENTRIES:   # the geometry and search families run through every projection entry
        for need in ("depth-zero", "image-edge", "dist-min", "dist-max", "view-half", "scale-clamp-high",
                     "proj-expression", "sum-order", "flags", "window-edge", "window-cells", "tie-first-wins",
                     "scale-clamp-low", "level-gate-L0", "level-gate-L1", "level-gate-L7", "chi2-stereo-7.8",
                     "chi2-mono-5.99", "no-uright", "fuse-dist-256") + tuple(f"scale-boundary-L{k}" for k in range(8)):
            assert need in by_entry[e], (e, need)
        pose = ("pose-order-sim3pair",) if e.startswith("sim3") else ("pose-order-se3", "pose-order-sim3")
        assert set(pose) <= by_entry[e], e
        assert all("pose-order" in c.variants for c in CASES if c.entry == e and family(c) in pose)
    for e in ("fuse", "fuse-sim3"):
        assert "best-dist-reported" in by_entry[e]
    assert any("log-all-double" in c.variants for c in CASES if c.name.startswith("scale-boundary"))
    for e in ("sbp", "sbp-kfs"):
        assert {"ladder-2", "ladder-3", "ladder-40", "preheld", "fallback-over-threshold"} <= by_entry[e]
    assert all(c.variants for c in CASES if c.name.startswith("ladder") and "reversed" not in c.name)


@pytest.mark.parametrize("entry", ["sim3", "sim3-rev"])
def test_sim3_pair_tells_its_poses_apart(entry):
    """The SearchBySim3 pose family has no symmetry to hide behind: S12 and S21 swapped, the keyframe
    poses swapped, the log scale factors swapped, and pKF2's intrinsics for pKF1's each change the output."""
    case = next(c for c in CASES if c.name == f"pose-order-sim3pair-{entry}")
    want = P.run_definition(case)[0]
    assert want[0] >= 1

    def run(**kw):
        c = P._clone(case, case.name)
        c.__dict__.update(kw)
        return P.run_definition(c)[0]

    def cam_with(base, **kw):
        c = type(base)()
        c.Tcw, c.fx, c.fy, c.cx, c.cy, c.log_scale_factor = base.Tcw, base.fx, base.fy, base.cx, base.cy, \
            base.log_scale_factor
        c.Ow[:] = base.Ow[:]
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    c1, c2 = case.cam, case.cam2
    assert not P.same(run(S12=case.S21, S21=case.S12), want)
    assert not P.same(run(cam=cam_with(c1, Tcw=c2.Tcw), cam2=cam_with(c2, Tcw=c1.Tcw)), want)
    assert not P.same(run(cam=cam_with(c1, log_scale_factor=c2.log_scale_factor),
                          cam2=cam_with(c2, log_scale_factor=c1.log_scale_factor)), want)
    assert not P.same(run(cam=cam_with(c1, fx=c2.fx, fy=c2.fy, cx=c2.cx, cy=c2.cy)), want)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(oracle_lib, case):
    out_d, tr = P.run_definition(case)
    out_o = P.run_oracle(oracle_lib, case)
    assert P.same(out_o, out_d), (out_o, out_d)
    case.check(case, tr, out_d)
    for v in case.variants:
        assert not P.same(P.run_definition(case, (v,))[0], out_d), f"the {v} evaluation no longer differs"
    for padded in (P.pad_keys(case), P.pad_points(case)):
        out_p, tr_p = P.run_definition(padded)
        out_po = P.run_oracle(oracle_lib, padded)
        assert P.same(out_po, out_p)
        assert out_p[0] == out_d[0]
        for a, b in zip(out_p[1:], out_d[1:]):
            np.testing.assert_array_equal(a[:len(b)], b)
            assert (a[len(b):] == -1).all()
        case.check(padded, tr_p, out_p)
