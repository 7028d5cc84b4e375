"""CPU: the planted kNN + ratio cases (tests/knn_patterns.py) through the definition
(oracle/knn_definition.py) and the C++ oracle. For every case the oracle's train rows, distances and count
equal the definition's and the case's own `check` proves on the trace that the case reaches what it names;
the inventory names every group; the ratio facts the cases stand on are asserted (at 0.7 the three ways of
evaluating the test and the integer test agree everywhere, at the other ratios the pairs on which they
differ are exactly the pairs planted); and embedding a case into a slab frame, at any of the geometries the
GPU test uses, changes no planted slot and answers no other. No case is skipped."""
import numpy as np
import pytest

import knn_patterns as P
from oracle import knn_definition as kd

CASES = P.all_cases()


def test_definition_basics():
    z = np.zeros(32, np.uint8)
    assert kd.hamming(z, P.row(range(256))) == 256 and kd.hamming(P.row([0, 37, 255]), z) == 3
    for k in range(256):   # the planted bit order deals the bits over the eight words
        r = P.row(P.ORDER[:k + 1]).view(np.uint32)
        assert [bin(int(w)).count("1") for w in r] == [(k + 1) // 8 + (1 if w < (k + 1) % 8 else 0) for w in range(8)]
    assert kd.top2(z, np.zeros((0, 32), np.uint8)) == (kd.INF, kd.INF, -1)
    assert kd.top2(z, [z]) == (0, kd.INF, 0)
    assert kd.top2_trace(z, [P.row([1, 2]), z, z, P.row([3])]) == (0, 0, 1, 2)   # the earlier of two equal rows
    assert kd.top2_trace(z, [P.row([1]), P.row([2]), z]) == (0, 1, 2, 0)          # the displaced best is second
    t, d, n = kd.knn_ratio([z], [z], 0.7)
    assert (t[0], d[0], n) == (-1, -1, 0)


def test_ratio_facts():
    """At 0.7 nothing tells the evaluations apart; at the other ratios exactly the planted pairs do."""
    for b in range(257):
        for a in range(b + 1):
            got = {kd.ratio_passes(a, b, 0.7, v) for v in kd.VARIANTS} | {10 * a < 7 * b, P.exact_passes(a, b, 0.7)}
            assert len(got) == 1, (a, b)
    assert P.disagreement(0.7) == set()
    assert P.ladder_pairs() <= P.planted_pairs("ladder-0.7")
    for d1 in range(2, 257):   # the ladder holds the last passing and the first failing d0 of every d1
        d0 = max(a for a in range(d1 + 1) if 10 * a < 7 * d1)
        assert {(d0, d1), (d0 + 1, d1)} <= P.planted_pairs("ladder-0.7") and not 10 * (d0 + 1) < 7 * d1
    for r in P.RATIOS:
        diff = {(a, b) for b in range(257) for a in range(b + 1)
                if len({kd.ratio_passes(a, b, r, v) for v in kd.VARIANTS}) > 1}
        d0, d1 = P.EQ_PAIR[r]
        near = {(d0 - 1, d1), (d0, d1)} | ({(d0 + 1, d1)} if d0 < d1 else set())
        assert P.planted_pairs(f"ratio-{r}") == diff | near, r
        for a, b in diff | near:   # the kernels' rule is the exact one
            assert kd.ratio_passes(a, b, r) == P.exact_passes(a, b, r)
        assert kd.ratio_passes(d0 - 1, d1, r) and not kd.ratio_passes(min(d0 + 1, d1), d1, r)
    # a float product is told from the kernels' rule at two ratios (the GPU suite relies on one at least)
    for r in (0.6, 0.8):
        assert any(kd.ratio_passes(a, b, r, "float") != kd.ratio_passes(a, b, r) for a, b in P.planted_pairs(f"ratio-{r}"))
    assert not exact_equal_passes()


def exact_equal_passes():
    """Exact equality rejects: 0.5, 0.75 and 1.0 are floats, so d0 == d1 * ratio exactly."""
    return [r for r in (0.5, 0.75, 1.0) if kd.ratio_passes(*P.EQ_PAIR[r], r)
            or P.EQ_PAIR[r][0] != P.EQ_PAIR[r][1] * r]


def test_case_inventory():
    names = {c.name for c in CASES}
    need = [f"tie-W{W}-{w}-{d}" for W in (4, 16) for w in ("same", "adjacent", "first-last")
            for d in ("d0", "d5", "distinct")]
    need += [f"tie-knn2-{a}-{b}-d{d}" for a, b in ((255, 256), (0, 511)) for d in (0, 5)]
    need += [f"merge-nt{nt}-{v}" for nt in (2, 3, 4, 5, 15, 16, 17, 19, 67) for v in "ab"]
    need += [f"merge-nt{nt}-c" for nt in (3, 4, 5, 15, 16, 17, 19, 67)]
    need += ["train-0", "train-1", "queries-0", "queries-1", "chunk-zero-query", "big-train-4096"]
    need += [f"chunk-nr{n}" for n in (255, 256, 257, 512, 513)] + [f"chunk-nl{n}" for n in (1, 255, 256, 257)]
    need += ["ladder-0.7-delta0", "ladder-0.7-delta1", "ladder-0.7-delta77", "ratio-1.0-delta0", "ratio-0.5-delta64"]
    for n in need:
        assert n in names, n
    assert P.MERGE_NT == [2, 3, 4, 5, 15, 16, 17, 19, 67]
    groups = {c.group for c in CASES}
    assert groups == {"ladder-0.7", "tie", "merge", "small", "chunk", "geometry"} | {f"ratio-{r}" for r in P.RATIOS}
    assert len(CASES) < 700   # k_knn2 takes one call per case
    # nt = 2 under W = 16 leaves 14 ranges empty, range 0 among them
    rg = P.wave_ranges(2, 16)
    assert sum(b > a for a, b in rg) == 2 and rg[0] == (0, 0)
    # the merge cases plant (5, 9) and (6, 7) in both orders of a pair of rows, in every nt
    for nt in P.MERGE_NT:
        plans = [p for c in CASES if c.name.startswith(f"merge-nt{nt}-") for p in c.facts["plan"]]
        for tgt in ((5, 9), (6, 7)):
            rows = {(p[2], p[3]) for p in plans if p[:2] == tgt}
            assert rows and all((b, a) in rows for a, b in rows), (nt, tgt)
        if nt <= 19:   # every ordered pair of rows
            assert {(p[2], p[3]) for p in plans} == {(a, b) for a in range(nt) for b in range(nt) if a != b}
        for W in (4, 16):   # the best in the first non-empty range and the second in the last, and the reverse
            live = [w for w, (a, b) in enumerate(P.wave_ranges(nt, W)) if b > a]
            where = lambda j: next(w for w, (a, b) in enumerate(P.wave_ranges(nt, W)) if a <= j < b)   # noqa: E731
            spans = {(where(p[2]), where(p[3])) for p in plans}
            assert {(live[0], live[-1]), (live[-1], live[0])} <= spans, (nt, W)
            if len(live) < nt:   # both of the top two in one later range
                assert any(a == b and a != live[0] for a, b in spans), (nt, W)
    # the geometry the frames cover
    frames = P.all_frames()
    assert {f.cap for f in frames} >= set(P.CAPS)
    base = [f for f in frames if f.case.name == P.GEOMETRY_BASE]
    assert {f.monoL for f in base} >= {0, 1, 63, 64, 65} and {f.monoR % 64 for f in frames} >= {0, 1, 63}
    assert any(f.nL - f.monoL == 0 and f.monoL > 0 for f in frames) and any(f.nL - f.monoL == 1 and f.monoL > 64 for f in frames)
    blocks = lambda f: [(q, q + P.KNN_Q) for q in range(0, f.cap, P.KNN_Q)]   # noqa: E731
    assert any(b <= f.monoL for f in base for a, b in blocks(f))                      # a block below monoL
    assert any(a < f.monoL < b for f in base for a, b in blocks(f))                   # across monoL
    assert any(a < f.nL < b for f in base for a, b in blocks(f))                      # across nL
    assert any(a >= f.nL for f in base for a, b in blocks(f))                         # past nL
    assert any(f.cap == 4096 and f.nR == 4096 and f.nL - f.monoL < 100 for f in frames)
    assert all(f.nL - f.monoL <= 400 for f in frames if f.cap > 2048)
    assert any(f.cap % 64 for f in frames)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(oracle_lib, case):
    t_d, d_d, n_d, tr = P.run_definition(case)
    n_o, t_o, d_o = oracle_lib.stereo_knn_ratio(case.L, case.R, case.ratio)
    assert n_o == n_d == int((t_d >= 0).sum())
    np.testing.assert_array_equal(t_o, t_d)
    np.testing.assert_array_equal(d_o, d_d)
    assert len(tr) == len(case.L)
    case.check(case, tr, t_d, d_d, n_d)


def _check_frame(oracle_lib, fr):
    c = fr.case
    cl, dl, cr, dr = fr.built()
    l2r, dist, n = kd.knn_frame(cl, dl, cr, dr, fr.cap, c.ratio)
    o_l2r, o_dist, o_n = fr.expected(oracle_lib)
    np.testing.assert_array_equal(o_l2r, l2r, err_msg=fr.name)
    np.testing.assert_array_equal(o_dist, dist, err_msg=fr.name)
    assert o_n == n
    t, d, n0, _ = P.run_definition(c)
    assert n == n0, fr.name
    np.testing.assert_array_equal(l2r[fr.monoL:fr.nL], np.where(t >= 0, t + fr.monoR, -1), err_msg=fr.name)
    np.testing.assert_array_equal(dist[fr.monoL:fr.nL], d, err_msg=fr.name)
    for a in (l2r, dist):
        assert (a[:fr.monoL] == -1).all() and (a[fr.nL:] == -1).all(), fr.name
    # the poison is in place: outside their ranges the train side holds the queries, the query side train rows
    if len(c.L) and fr.monoR:
        np.testing.assert_array_equal(dr[0], c.L[0])
    if len(c.R) and fr.nL < fr.cap:
        np.testing.assert_array_equal(dl[fr.cap - 1], c.R[(fr.cap - 1) % len(c.R)])


def test_padding_facts(oracle_lib):
    """Every frame the GPU test launches: the planted slots are the case's, shifted by monoR; no other slot
    answers."""
    for fr in P.all_frames():
        _check_frame(oracle_lib, fr)


@pytest.mark.parametrize("name", ["merge-nt5-a", "tie-W4-adjacent-d0", "ladder-0.7-delta3", "train-1"])
def test_padding_every_geometry(oracle_lib, name):
    """A few cases at every listed monoL with every listed cap."""
    c = P.case(name)
    for cap in P.CAPS:
        for monoL in (0, 1, 63, 64, 65):
            if monoL + len(c.L) <= cap:
                _check_frame(oracle_lib, P.Frame(c, monoL, (monoL * 7 + 1) % 67, cap))


@pytest.mark.parametrize("addressing", P.ADDRESSINGS)
def test_pack_addressing(addressing):
    frames = P.frames_by_cap()[100][:5]
    cl, dl, cr, dr, (lb, ls, rb, rs) = P.pack(frames, addressing)
    assert (cl is cr) == (addressing == "interleaved") and len(cl) == len(dl) and len(cr) == len(dr)
    assert addressing == "interleaved" or len(cl) != len(cr)
    for f, fr in enumerate(frames):
        a, b, c, d = fr.built()
        for got, want in ((cl[lb + f * ls], a), (dl[lb + f * ls], b), (cr[rb + f * rs], c), (dr[rb + f * rs], d)):
            np.testing.assert_array_equal(got, want)
    for chunk in P.launches(P.frames_by_cap()[4096], 17):
        assert len(chunk) == 17 and all(a is not b for a, b in zip(chunk, chunk[1:]))
