"""CPU: every planted case of tests/frustum_patterns.py. The definition (oracle/frustum_definition.py) equals
the C++ oracle bit for bit (is_in_frustum, search_local_points with and without a rig, sbp_lastframe_pose), the
case's check proves from the trace that its rule decided, and every careless variant the case names disagrees."""
import numpy as np
import pytest

import frustum_patterns as P
from oracle import frustum_definition as fd
from orb_slam3_ros_amd.matcher import MP_IN_VIEW

FRUSTUM = P.by_kind("frustum")
LAST = P.by_kind("last")


@pytest.fixture(scope="module")
def om(oracle_lib):
    return oracle_lib


def test_every_family_has_cases_and_sensitive_ones_name_variants():
    for fam in P.FAMILIES:
        cs = [c for c in P.CASES if c.family == fam]
        print(f"{fam}: {len(cs)} cases, {sum(len(c.pts) for c in cs)} points, variants "
              f"{sorted({v for c in cs for v in c.variants})}")
        assert cs
    assert len({c.name for c in P.CASES}) == len(P.CASES)
    for fam in ("bounds", "distance", "cosine", "sums"):   # the float-sensitive families
        assert all(c.variants for c in P.CASES if c.family == fam), fam
    for name in ("depth-zeros-kb8", "scale-boundaries", "rig-two-views", "rig-right-view-bounds", "kb8-axis-and-right-angle",
                 "last-se3-rotated", "last-two-cameras-trl"):
        assert [c for c in P.CASES if c.name == name][0].variants, name
    assert all(v in fd.VARIANTS for c in P.CASES for v in c.variants)


@pytest.mark.parametrize("c", FRUSTUM, ids=repr)
def test_frustum_case(om, c):
    ntm, rec, tr = c.define()
    c.check(c, tr, rec)
    on, orec = om.is_in_frustum(c.geom, c.cam, c.flagged(), c.rig)
    assert on == ntm
    nan = np.zeros(len(rec), bool)
    for k in rec.dtype.names:
        if rec[k].dtype.kind == "f":
            nan |= np.isnan(orec[k]) | np.isnan(rec[k])
    assert np.nonzero(nan)[0].tolist() == list(c.nan)          # exactly the named points are relaxed
    P.assert_records_equal(rec, orec, c.nan)
    for v in c.variants:
        vn, vrec, _ = c.define(v)
        assert vrec.tobytes() != rec.tobytes(), f"variant {v} agrees on {c.name}"
    if c.nan:
        return
    # the fused search on keypoints planted around every point in view, at the predicted level +- 1
    F = P.amplify(c, rec)
    mvp, obs = np.full(F.N, -1, np.int32), np.zeros(F.N, np.int32)
    n, ntm2 = om.search_local_points(F, c.cam, c.flagged(), mvp, obs, c.th, False, 50.0, 0.8, c.rig)
    want = np.full(F.N, -1, np.int32)
    wn = om.OracleMatcher(0.8).sbp_local(F, want, np.zeros(F.N, np.int32), rec, c.th) if ntm else 0
    assert (n, ntm2) == (wn, ntm)
    np.testing.assert_array_equal(mvp, want)
    assert ntm == 0 or n > 0
    if c.family == "compaction" and 0 < ntm <= 2048 and not hasattr(c, "winner"):
        seen = np.nonzero(rec["flags"] & MP_IN_VIEW)[0]
        assert rec["id"][seen[-1]] in mvp                          # the last compacted record decides a slot
    if hasattr(c, "winner"):
        assert (mvp >= 0).sum() == 1 and mvp.max() == c.winner
        a, b = np.nonzero(rec["flags"] & MP_IN_VIEW)[0]
        sw = c.flagged()
        sw[[a, b]] = sw[[b, a]]
        m2 = np.full(F.N, -1, np.int32)
        om.search_local_points(F, c.cam, sw, m2, np.zeros(F.N, np.int32), c.th, False, 50.0, 0.8, c.rig)
        assert m2.max() != c.winner                            # swapping the pair changes the row


def last_rows(om, c, rec, ruv):
    mvp, obs = np.full(c.F.N, -1, np.int32), np.zeros(c.F.N, np.int32)
    m = om.OracleMatcher(0.9, False)
    if c.Trl is not None:
        n = m.sbp_lastframe_stereo(c.F, mvp, obs, rec, ruv, c.th, c.fw, c.bw)
    else:
        n = m.sbp_lastframe(c.F, mvp, obs, rec, c.th, c.fw, c.bw)
    return n, mvp


@pytest.mark.parametrize("c", LAST, ids=repr)
def test_last_frame_case(om, c):
    rec, ruv, tr = c.define()
    c.check(c, tr, rec)
    assert c.F.N <= 64
    n, row = last_rows(om, c, rec, ruv)
    np.testing.assert_array_equal(row, c.want)                 # the inner keypoints, nothing on the edge
    mvp, obs = np.full(c.F.N, -1, np.int32), np.zeros(c.F.N, np.int32)
    on = om.OracleMatcher(0.9, False).sbp_lastframe_pose(c.F, mvp, obs, c.pts, c.Tcw, c.model, c.th, c.fw, c.bw, c.Trl)
    assert on == n == int((c.want >= 0).sum())
    np.testing.assert_array_equal(mvp, row)
    # one ulp of the definition's u or v, or of the right centre's, either way, changes the expected row
    assert c.amplified
    for i in c.amplified:
        for k, key in enumerate(("u", "v")):
            for sgn in (-1, 1):
                r2 = rec.copy()
                r2[key][i] = P.step(rec[key][i], sgn)
                assert not np.array_equal(last_rows(om, c, r2, ruv)[1], row), (c.name, i, key, sgn)
                if c.Trl is not None:
                    q2 = ruv.copy()
                    q2[i, k] = P.step(ruv[i, k], sgn)
                    assert not np.array_equal(last_rows(om, c, rec, q2)[1], row), (c.name, i, key, sgn, "right")
    for v in c.variants:
        vrec, vruv, _ = c.define(v)
        assert vrec.tobytes() != rec.tobytes() or vruv.tobytes() != ruv.tobytes(), f"variant {v} agrees on {c.name}"
