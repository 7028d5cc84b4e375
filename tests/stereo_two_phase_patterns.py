"""Planted ComputeStereoMatches cases for the two-phase form of k_stereo (phase A: match and compact the
keys that reach the window search into a work list; phase B: the SAD refinement over that list, 16 lanes
per item, 64 items per block round, the next round's window rows loaded ahead). Built on
tests/stereo_patterns.py; each case asserts on the CPU, from the trace of oracle/stereo_definition.py,
that it reaches its branch.

A key is on the work list iff the definition read its windows (`KeyTrace.window`): it had a candidate, a
best distance below 75 and passed `iniu < 0 || endu >= w`. A block's list holds the listed keys among its
LK left keys, LK = 512 in the batch form and 16 in the small form.
"""
from __future__ import annotations

import numpy as np

import stereo_patterns as sp

F32 = np.float32
ST_LK, SMALL_LK = 512, 16   # orbfe_kernels.hip ST_LK, orbfe_engine.hip kSmallStereoLk
GROUP, ROUND = 4, 64        # items per wave iteration (16 lanes each) and per block round (16 waves)


def list_lengths(tr, lk):
    """Work-list length of every block of lk left keys."""
    listed = [k.window is not None for k in tr.keys]
    return [sum(listed[i:i + lk]) for i in range(0, len(listed), lk)]


def _unmatched(b, i):
    """A left key alone on its rows: no right band reaches rows 200 .. 240."""
    return b.add("L", 0, sp.EDGE + 3 * i, 200 + (i % 3) * 20)


def list_case(m):
    """m true matches (level 0, 10 per row, rows 15 apart) behind and between left keys without a
    candidate: the list has m entries and its indices differ from the key indices. Up to m = 5 the whole
    frame is one block in either form."""
    b = sp.Build(f"list-{m}")
    _unmatched(b, 0)
    for i in range(m):
        if i % 2 == 1 and len(b.k["L"]) < SMALL_LK - m:
            _unmatched(b, 1 + i)
        b.pair(0, 100 + 20 * (i % 10), 30 + 15 * (i // 10), sp.SHIFT, 2)
    _unmatched(b, 50)

    def pre(c, ref):
        tr = ref["def"][3]
        assert list_lengths(tr, ST_LK) == [m], list_lengths(tr, ST_LK)
        if m <= 5:
            assert len(tr.keys) <= SMALL_LK and list_lengths(tr, SMALL_LK) == [m]
        else:   # the small form: several blocks, one of them with a full list
            assert max(list_lengths(tr, SMALL_LK)) == SMALL_LK
        assert tr.keys[0].outcome == "no-candidates" and tr.keys[-1].outcome == "no-candidates"
        assert sum(k.outcome in ("accepted", "cut") for k in tr.keys) >= (m + 1) // 2
    return sp.case(f"list-{m}", b, pre)


def window_out_case(valid):
    """Left keys whose only candidate is a right key on a negative column (OUTSIDE the extractor's domain,
    as in stereo_patterns.edge_reject): they match, and `iniu < 0` keeps them off the list. With
    `valid`, true matches sit between them, so list index and key index part."""
    name = "window-out-mixed" if valid else "window-out-all"
    b = sp.Build(name)
    want = []
    for i in range(9):
        d = b.desc()
        y = 30 + 12 * i
        b.add("L", 0, 40 + i, y, d)
        b.add_raw("R", -3.0 - i, float(y), 0, b.flip(d, 2))
        want.append("window-out")
        if valid and i % 2 == 0:
            b.pair(0, 150 + 10 * i, y + 6, sp.SHIFT, 2)
            want.append(None)

    def pre(c, ref):
        tr = ref["def"][3]
        got = sp.outcomes(tr)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g == w if w else g in ("accepted", "cut"), got
        assert all(k.best_dist == 2 for k in tr.keys)
        if valid:
            listed = [i for i, k in enumerate(tr.keys) if k.window is not None]
            assert len(listed) == 5 and all(i != n for n, i in enumerate(listed))
        else:
            assert list_lengths(tr, ST_LK) == [0] and ref["def"][2] == 0
    return sp.case(name, b, pre, outside="right keys on negative columns: rejected by iniu < 0 before any pixel is read")


def tie_scan_case():
    """Two candidates on the best distance in a band of more than 64 candidates. A scan of 16 (or 64)
    lanes meets the lower right index in an earlier trip for one left key and in a later trip for the
    other: the lowest iR must win both."""
    b = sp.Build("tie-scan")
    yb = 120

    def tied(x, dy_true, dy_decoy):
        d = b.desc()
        i_l = b.add("L", 0, x, yb, d)
        return i_l, b.add("R", 0, x - sp.SHIFT, yb + dy_true, b.flip(d, 6)), b.add("R", 0, x - 60, yb + dy_decoy, b.flip(d, 6))
    early = tied(200, -2, 2)   # the lower index starts its band 4 rows earlier
    late = tied(240, 2, -2)    # the lower index starts its band 4 rows later
    b.fill_right(70, [yb - 1], x0=sp.EDGE + 1)   # 70 records sort between the two band starts

    def pre(c, ref):
        tr, alt = ref["def"][3], ref["def-tie-last"]
        for i_l, first, second in (early, late):
            kt = tr.keys[i_l]
            assert kt.nties == 2 and kt.best_dist == 6 and kt.best_idx == first < second
            assert kt.ncand > 64 and kt.window is not None
            assert ref["def"][0][i_l] != alt[0][i_l], "either tie rule gives the same answer"
        for stride in (16, 64):
            def trips(i_l, i_r):
                lo, hi = sp.scan_pos(c, i_l, i_r)
                return lo // stride, hi // stride
            i_l, first, second = early
            assert trips(i_l, first)[1] < trips(i_l, second)[0]
            i_l, first, second = late
            assert trips(i_l, first)[0] > trips(i_l, second)[1]
    return sp.case("tie-scan-trips", b, pre, tie_last=True)


def count_above_lk(extra):
    """N = ST_LK + extra: the frame's second block holds `extra` left keys."""
    c = sp.count_case(ST_LK + extra, name=f"N-lk-plus-{extra}")
    inner = c.pre

    def pre(c, ref):
        inner(c, ref)
        tr = ref["def"][3]
        lens = list_lengths(tr, ST_LK)
        assert len(tr.keys) == ST_LK + extra and len(lens) == 2
        assert lens[0] > ROUND and lens[0] % ROUND != 0 and 1 <= lens[1] <= extra, lens
    c.pre = pre
    return c


def mixed_levels_case():
    """Neighbouring list items on different levels, level 0 among them, on caller images with an odd pitch
    and base offset: the rows loaded ahead for one item must never serve another. More than one round of
    items in the batch form."""
    b = sp.Build("mixed-levels")
    sp.generic_keys(b, 150)

    def pre(c, ref):
        tr = ref["def"][3]
        lv = [k.window[0] for k in tr.keys if k.window is not None]
        assert len(lv) > ROUND and len(lv) % ROUND != 0, len(lv)
        change = [(a, z) for a, z in zip(lv, lv[1:]) if a != z]
        assert len(change) >= len(lv) // 2 and any(0 in p for p in change) and len(set(lv)) >= 5, (len(change), set(lv))
        # items one round apart share a lane group in consecutive rounds
        assert sum(a != z for a, z in zip(lv, lv[ROUND:])) >= 1
        assert sum(k.outcome in ("accepted", "cut") for k in tr.keys) >= 30
    return sp.case("mixed-levels-odd-pitch", b, pre, layout=(13, 3))


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = [list_case(m) for m in (0, 1, 2, 3, GROUP + 1, ROUND + 1)] + [
            window_out_case(False), window_out_case(True), tie_scan_case(),
            sp.count_case(0, name="two-phase-N-0"), sp.count_case(40, 0, "two-phase-Nr-0"), count_above_lk(3),
            mixed_levels_case(),
        ]
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES
