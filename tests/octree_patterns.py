"""Seeded adversarial key sets for DistributeOctTree (k_octree), and the CPU preconditions that prove
each one reaches the branch it is named for. Shared by tests/test_octree_definition.py (CPU) and
tests/test_gpu_octree_adversarial.py (GPU); nothing here touches a GPU.

A case is an OctCase(name, img, ..., lap, pre). pre(case, levels) gets, per pyramid level, the pair
(result keys, Trace) of oracle/octree_definition.py run on that level's keys, and asserts from it
alone that the case reaches its branch, for the thread count(s) it names. Key sets are planted as
isolated impulses on a flat background (an impulse of contrast c is one key of score c - 1, see
fast_patterns.py), at least 7 px apart; noise images supply thousands of keys where needed.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import fast_patterns as fp
from oracle import fast_definition as fd
from oracle import octree_definition as od

B = fd.BORDER

# ---- the engine's thresholds, and where they come from ------------------------------------------
# orbfe_engine.hip: a launch of fewer than kSmallBatch = 16 images (every host call) runs
#   k_octree<kSmallOctNt = 1024>, a larger batch k_octree<OCT_NT = 256>.
# orbfe_kernels.hip, k_octree<NT>:
#   regk  = NT >= 1024 && K <= NT * 8     keys of the level in registers, 8 per thread; else the
#                                         global lkeys / nodeof lists (always at NT = 256)
#   fini  = regk && nIni <= NT            one thread per root column; else the scanned roots
#   phase-1 step fused iff n <= NT        (n: nodes in the list at the top of the step)
#   phase-2 step fused iff m <= NT && n <= NT   (m: expandable nodes the last step pushed)
#   lapping ranks: one packed scan iff n <= NT, two scans otherwise
#   node capacity NC = max over levels of max(N + 3, 4 nIni) + 8 (build_geom); the octree's LDS
#   (94 bytes per node) must fit 160 KiB, which bounds a level's budget N near 1730
NT_BATCH, NT_HOST = 256, 1024
KEYS_PER_THREAD = 8
SMALL_BATCH = 16


def branches(levels, nt):
    """The k_octree<nt> paths the levels of a case take, derived from the definition's traces."""
    s = set()
    for out, tr in levels:
        regk = nt >= NT_HOST and tr.K <= nt * KEYS_PER_THREAD
        s.add("keys-in-registers" if regk else "keys-in-global-lists")
        s.add("roots-per-thread" if regk and tr.n_ini <= nt else "roots-scanned")
        n, m = tr.roots, 0
        for r in tr.rounds:
            if r.phase == 1:
                s.add("p1-fused" if n <= nt else "p1-generic")
            elif m <= nt and n <= nt:
                s.add("p2-fused")
            else:
                s.add("p2-generic-m" if m > nt else "p2-generic-n")
            if r.finish == "reach-N":
                s.add(f"finish-p{r.phase}-reach-N")
            elif r.finish == "stall":
                s.add("finish-stall-cluster" if len(out) < tr.K else "finish-stall-singles")
            n, m = r.n, r.m
        s.add("ranks-one-scan" if n <= nt else "ranks-two-scans")
    return s


def need(case, levels, nt, *want):
    got = branches(levels, nt)
    assert set(want) <= got, f"{case.name}: k_octree<{nt}> wanted {want}, the definition shows {sorted(got)}"


@dataclass
class OctCase(fp.Case):
    lap: tuple = (0, 0)
    ini: int = 20
    min: int = 7
    nlevels: int = 1

    def __repr__(self):
        return self.name


def case(name, img, nfeat, pre, nlevels=1, lap=(0, 0), ini=20, mn=7):
    return OctCase(name=name, img=img, ini=ini, min=mn, nlevels=nlevels, scale=1.2, nfeat=nfeat, pre=pre, lap=lap)


# ---- planted keys -------------------------------------------------------------------------------
def impulses(w, h, pts):
    """Image of w x h with a bright impulse of contrast c at every (x, y, c) of pts, coordinates
    relative to the level's border as the octree sees them."""
    img = np.zeros((h, w), np.uint8)
    for x, y, c in pts:
        assert 3 <= x < w - 2 * B - 3 and 3 <= y < h - 2 * B - 3, (x, y)
        img[y + B, x + B] = c
    return img


def planted(case_, levels, pts):
    """Level 0 of the case holds exactly the planted keys (the definition saw them all)."""
    _, lists = fd.cell_keys(case_.img, case_.ini, case_.min)
    got = sorted(k for l in lists for k in l)
    assert got == sorted((x, y, c - 1) for x, y, c in pts), f"{case_.name}: FAST keys differ from the planted ones"
    assert levels[0][1].K == len(pts)


def lattice(side, multi, seed):
    """side x side cells of 15 x 15 px (a detection area of 15 side, a power of two times 15, so the
    tree's cells are the lattice's after log2(side) rounds). Every cell holds one key at offset
    (4, 4), except the `multi` cells (col, row), which hold three: A (0, 1) and B (7, 1) share the
    8 x 8 child and part at the next split, C (8, 9) leaves at once."""
    rng = np.random.default_rng(seed)
    pts = []
    for r in range(side):
        for c in range(side):
            x0, y0 = 15 * c, 15 * r
            if (c, r) in multi:
                pts += [(x0, y0 + 1, int(rng.integers(30, 250))), (x0 + 7, y0 + 1, int(rng.integers(30, 250))),
                        (x0 + 8, y0 + 9, int(rng.integers(30, 250)))]
            else:
                pts.append((x0 + 4, y0 + 4, int(rng.integers(30, 250))))
    return impulses(15 * side + 2 * B, 15 * side + 2 * B, pts), pts


def multi_block(side, cols, rows):
    """`cols` lattice columns x `rows` lattice rows of multi cells, clear of the first row / column."""
    step = (side - 2) // cols
    return {(1 + step * i, 1 + j) for i in range(cols) for j in range(rows)}


# ---- phase-1 / phase-2 step forms ---------------------------------------------------------------
def _lattice_case(name, side, cols, rows, nfeat, pre):
    multi = multi_block(side, cols, rows)
    img, pts = lattice(side, multi, 10 * side + cols)

    def chk(c, levels):
        planted(c, levels, pts)
        pre(c, levels)
    return case(name, img, nfeat, chk)


def pre_p1_generic(nt):
    def pre(c, levels):
        tr = levels[0][1]
        need(c, levels, nt, "p1-generic", "p1-fused", "finish-stall-singles", "ranks-two-scans")
        # a generic step that divides nodes, not only the final one that finds nothing to divide
        assert _generic_divides(tr, nt), c.name
        assert all(r.phase == 1 for r in tr.rounds) and len(levels[0][0]) == tr.K < tr.N
    return pre


def _generic_divides(tr, nt):
    n = tr.roots
    for r in tr.rounds:
        if r.phase == 1 and n > nt and r.divided > 0:
            return True
        n = r.n
    return False


def pre_p2_generic_n(nt):
    def pre(c, levels):
        tr = levels[0][1]
        need(c, levels, nt, "p2-fused", "p2-generic-n", "finish-p2-reach-N")
        p2 = [r for r in tr.rounds if r.phase == 2]
        # the first walk runs to t = m without reaching N; the second breaks inside a tie group
        assert len(p2) == 2 and p2[0].break_at is None and p2[0].divided == p2[0].sorted_m
        assert p2[1].sorted_m <= nt and p2[1].tie_group and p2[1].break_in_tie and 0 < p2[1].break_at < p2[1].sorted_m - 1
    return pre


def pre_p2_generic_m(nt):
    def pre(c, levels):
        need(c, levels, nt, "p2-generic-m", "finish-p2-reach-N")
    return pre


def step_cases():
    return [
        # 256 + 40 multi cells: rounds of 256 (fused) and 296, 336 nodes (generic at 256 threads); N = 420 keeps phase 1
        _lattice_case("p1-generic-256", 16, 4, 10, 420, pre_p1_generic(NT_BATCH)),
        _lattice_case("p1-generic-1024", 32, 4, 10, 1190, pre_p1_generic(NT_HOST)),
        # 60 multi cells in 6 columns: phase 2 at n = side^2; its first walk divides all 60 (+1 each), the
        # second starts above NT with m = 60 and breaks 14 divisions in, inside the (2, UL.x) group of a column
        _lattice_case("p2-generic-n-256", 16, 6, 10, 256 + 60 + 14, pre_p2_generic_n(NT_BATCH)),
        _lattice_case("p2-generic-n-1024", 32, 6, 10, 1024 + 60 + 14, pre_p2_generic_n(NT_HOST)),
        # noise under 3 (5) root columns: 192 (320) nodes stay in phase 1, the next round pushes more than NT
        case("p2-generic-m-256", fp.noise_image(31, 320, 128), 1000, pre_p2_generic_m(NT_BATCH)),
        case("p2-generic-m-1024", fp.noise_image(32, 512, 128), 1500, pre_p2_generic_m(NT_HOST)),
    ]


# ---- key storage --------------------------------------------------------------------------------
def pre_keys_global(c, levels):
    assert levels[0][1].K > NT_HOST * KEYS_PER_THREAD
    need(c, levels, NT_HOST, "keys-in-global-lists", "roots-scanned", "p2-fused")


def pre_keys_registers(c, levels):
    assert NT_HOST * KEYS_PER_THREAD - 1024 < levels[0][1].K <= NT_HOST * KEYS_PER_THREAD   # the last slot group is in use
    need(c, levels, NT_HOST, "keys-in-registers", "roots-per-thread")
    need(c, levels, NT_BATCH, "keys-in-global-lists", "roots-scanned")


def storage_cases():
    return [case("keys-global-host", fp.noise_image(41, 336, 336), 1100, pre_keys_global),
            case("keys-registers-full", fp.noise_image(42, 320, 316), 600, pre_keys_registers)]


# ---- K edge counts ------------------------------------------------------------------------------
def spread_points(n, w, h, seed, lo=30, hi=250):
    """n impulses on a pitch-9 lattice of the detection area, seeded choice of sites and contrasts."""
    rng = np.random.default_rng(seed)
    sites = [(x, y) for y in range(4, h - 2 * B - 4, 9) for x in range(4, w - 2 * B - 4, 9)]
    idx = rng.permutation(len(sites))[:n]
    return [(sites[i][0], sites[i][1], int(rng.integers(lo, hi))) for i in sorted(idx)]


def pre_k(k, finish, returned):
    def pre(c, levels):
        out, tr = levels[0]
        assert tr.K == k and len(out) == returned and tr.finish == finish, (c.name, tr.K, len(out), tr.finish)
    return pre


def pre_k0_level(c, levels):
    assert levels[0][1].K > 0 and levels[1][1].K == 0 and levels[1][0] == []
    assert levels[1][1].rounds[-1].finish == "stall"


def count_cases():
    out = []
    for name, k, nfeat, finish in (("k-1", 1, 300, "stall"), ("k-below-n", 23, 300, "stall"), ("k-equals-n", 23, 23, "reach-N")):
        pts = spread_points(k, 137, 102, 50 + k + nfeat)

        def chk(c, levels, pts=pts, k=k, finish=finish):
            planted(c, levels, pts)
            pre_k(k, finish, k)(c, levels)
        out.append(case(name, impulses(137, 102, pts), nfeat, chk))
    # contrasts 21, 22 at ini = min = 20: level 1's bilinear taps (at most 0.9 x 0.9 of the impulse) leave no corner
    pts = spread_points(40, 137, 102, 77, 21, 23)
    out.append(case("k-0-on-level-1", impulses(137, 102, pts), 300, pre_k0_level, nlevels=2, ini=20, mn=20))
    return out


# ---- finish reasons, phase-2 break positions ----------------------------------------------------
CLUSTER = [(10, 10, 60), (17, 10, 90), (10, 17, 75), (100, 20, 50), (100, 80, 40), (60, 60, 45)]


def pre_stall_cluster(c, levels):
    out, tr = levels[0]
    planted(c, levels, CLUSTER)
    need(c, levels, NT_HOST, "finish-stall-cluster")
    assert len(out) < tr.K < tr.N and (17, 10, 89) in out and (10, 10, 59) not in out


def pre_break_at_0(c, levels):
    p2 = [r for r in levels[0][1].rounds if r.phase == 2]
    assert len(p2) == 1 and p2[0].break_at == 0 and p2[0].sorted_m > 1


def pre_break_in_tie(c, levels):
    p2 = [r for r in levels[0][1].rounds if r.phase == 2]
    assert p2 and p2[-1].break_in_tie and p2[-1].finish == "reach-N"
    need(c, levels, NT_BATCH, "p2-fused")


def pre_p1_reach_n(c, levels):
    tr = levels[0][1]
    assert all(r.phase == 1 for r in tr.rounds) and tr.finish == "reach-N" and len(tr.rounds) > 1


def finish_cases():
    return [case("stall-cluster", impulses(160, 128, CLUSTER), 300, pre_stall_cluster),
            case("break-at-0", fp.noise_image(61, 160, 128), 65, pre_break_at_0),
            case("break-in-tie", fp.noise_image(62, 160, 128), BREAK_IN_TIE_N, pre_break_in_tie),
            case("p1-reach-n", fp.noise_image(63, 160, 128), 64, pre_p1_reach_n)]


BREAK_IN_TIE_N = 150   # found on the CPU: the budget at which noise_image(62)'s break splits a tie group


# ---- score ties ---------------------------------------------------------------------------------
# 137 x 102: FAST cells of 35 columns, the boundary between cells 0 and 1 at x = 38; the tree splits x at 53.
# P and Q, equal scores, share every tree node (the distribution stalls on them): P lies in FAST cell 0
# and so comes first in key order although Q is above it. R and S tie inside one FAST cell, in the other
# root column.
TIES = [(35, 20, 80), (42, 13, 80), (60, 45, 66), (67, 45, 66)]


def pre_score_tie_cells(c, levels):
    out, tr = levels[0]
    planted(c, levels, TIES)
    assert fd.bin_keys([35, 42], [20, 13], [79, 79], 137, 102)[0].tolist()[:2] == [1, 1]   # two FAST cells
    assert tr.score_tie_nodes == 2 and tr.finish == "stall"
    assert sorted(out) == [(35, 20, 79), (60, 45, 65)]


def pre_score_tie_noise(c, levels):
    out, tr = levels[0]
    assert tr.score_tie_nodes > len(out) // 2 and {s for _, _, s in out} == {254}


def tie_cases():
    rng = np.random.default_rng(71)
    return [case("score-tie-cells", impulses(137, 102, TIES), 300, pre_score_tie_cells),
            case("score-tie-binary-noise", (rng.integers(0, 2, (128, 160)) * 255).astype(np.uint8), 40, pre_score_tie_noise)]


# ---- root columns -------------------------------------------------------------------------------
def pre_n_ini(n_ini):
    def pre(c, levels):
        tr = levels[0][1]
        assert tr.n_ini == n_ini and tr.empty_roots == 0 and tr.K > 0, (c.name, tr.n_ini, tr.empty_roots)
    return pre


def pre_last_root(c, levels):
    tr = levels[0][1]
    assert tr.n_ini >= 3 and tr.empty_roots == tr.n_ini - 1 and tr.roots == 1 and tr.K > 4


def boundary_points(w, h):
    """Keys on x = (int)(hX (i + 1)) and its two neighbours for every inner root boundary, 30 rows apart,
    plus a few elsewhere."""
    n_ini, hx, cols = od.root_geometry(w - 2 * B, h - 2 * B)
    pts = []
    for i in range(n_ini - 1):
        for k, dx in enumerate((-1, 0, 1)):
            pts.append((cols[i][1] + dx, 5 + 15 * i + 30 * k, 40 + 10 * len(pts)))
    pts += [(10, 40, 100), (w - 2 * B - 10, 50, 120)]
    return pts


def pre_boundary(c, levels):
    h, w = c.img.shape
    out, tr = levels[0]
    pts = boundary_points(w, h)
    planted(c, levels, pts)
    n_ini, hx, cols = od.root_geometry(w - 2 * B, h - 2 * B)
    assert n_ini >= 3 and float(hx) != int(hx)
    assert sorted(tr.boundary_keys) == [(cols[i][1], i) for i in range(n_ini - 1)]
    # a boundary key belongs to the root on its left by x / hX while that root's rectangle ends before it
    assert all(od.root_of(x, hx) == i and not (cols[i][0] <= x < cols[i][1]) for x, i in tr.boundary_keys)
    assert len(out) == tr.K   # every key is isolated in the end


def root_cases():
    x_last = od.root_geometry(282 - 2 * B, 102 - 2 * B)[2][-1][0]
    last = [(x, y, c) for x, y, c in spread_points(90, 282, 102, 81) if x > x_last]
    return [case("n-ini-1", fp.noise_image(82, 120, 128), 100, pre_n_ini(1)),
            case("n-ini-2", fp.noise_image(83, 180, 102), 100, pre_n_ini(2)),
            case("n-ini-4", fp.noise_image(84, 310, 102), 100, pre_n_ini(4)),
            case("last-root-only", impulses(282, 102, last), 300, pre_last_root),
            case("root-boundary-fractional", impulses(282, 132, boundary_points(282, 132)), 300, pre_boundary)]


# ---- over-budget output -------------------------------------------------------------------------
def pre_over_budget(c, levels):
    out, tr = levels[0]
    assert 4 * tr.n_ini > tr.N and len(out) > tr.N + 3 and len(tr.rounds) == 1 and tr.finish == "reach-N"


def budget_cases():
    return [case("over-budget", fp.noise_image(91, 400, 90), 5, pre_over_budget)]


# ---- lapping ranks ------------------------------------------------------------------------------
def scaled_x(out, level, scale=1.2):
    """Output x of the level's result keys as operator() scales them: float32 x (+ border) times the
    float32 level scale (level 0 unscaled)."""
    s = np.float32(1.0)
    for _ in range(level):
        s = np.float32(np.float64(s) * np.float64(np.float32(scale)))
    x = np.asarray([k[0] for k in out], np.float32) + np.float32(B)
    return x if level == 0 else x * s


def lap_split(out, level, lap, scale=1.2):
    """(lapping, non-lapping) counts of a level's result keys; both ends of the area are inclusive."""
    sx = scaled_x(out, level, scale)
    inside = (sx >= np.float32(lap[0])) & (sx <= np.float32(lap[1]))
    return int(inside.sum()), int((~inside).sum())


def pre_lap_exact(nt, which):
    def pre(c, levels):
        for l, (out, tr) in enumerate(levels):
            sx = scaled_x(out, l)
            assert (sx == np.float32(c.lap[0])).any() and (sx == np.float32(c.lap[1])).any(), \
                f"{c.name}: level {l} has no key with scaled x on lap0 / lap1"
            nl, nm = lap_split(out, l, c.lap)
            assert nl > 0 and nm > 0
        need(c, levels, nt, which)
    return pre


def pre_lap_all(c, levels):
    assert all(lap_split(out, l, c.lap) == (len(out), 0) and out for l, (out, _) in enumerate(levels))


def pre_lap_none(c, levels):
    assert all(lap_split(out, l, c.lap) == (0, len(out)) and out for l, (out, _) in enumerate(levels))


# found on the CPU: values that are the scaled x of a result key on every level of the case. On level 1
# float32(x) * 1.2f is an integer only for some multiples of 5 (the product rounds back onto it).
LAP_SMALL, LAP_LARGE, LAP_HOST = (66, 132), (42, 168), (60, 190)


def lap_cases():
    a, b, c = fp.noise_image(101, 200, 160), fp.noise_image(102, 256, 200), fp.noise_image(103, 256, 200)
    return [case("lap-exact-one-scan", a, 300, pre_lap_exact(NT_BATCH, "ranks-one-scan"), nlevels=2, lap=LAP_SMALL),
            case("lap-exact-two-scans-256", b, 700, pre_lap_exact(NT_BATCH, "ranks-two-scans"), nlevels=2, lap=LAP_LARGE),
            case("lap-exact-two-scans-1024", c, 1100, pre_lap_exact(NT_HOST, "ranks-two-scans"), lap=LAP_HOST),
            case("lap-all", a, 300, pre_lap_all, nlevels=2, lap=(0, 4096)),
            case("lap-none", a, 300, pre_lap_none, nlevels=2, lap=(300, 400))]


def all_cases():
    return (step_cases() + storage_cases() + count_cases() + finish_cases() + tie_cases() + root_cases() +
            budget_cases() + lap_cases())


# ---- references ---------------------------------------------------------------------------------
def std_sort(oracle_lib):
    """The oracle's exported std::sort of u64 values by their high word, as the definition's `sort`."""
    lib = oracle_lib.lib()

    def sort(vals):
        a = np.asarray(vals, np.uint64)
        if len(a):
            lib.oro_std_sort_u64_hi(a.ctypes.data, len(a))
        return a.tolist()
    return sort


def run_definition(raw, w, h, n, sort):
    """The definition on one level: raw = the level's keys (x, y, score) in vToDistributeKeys order."""
    return od.distribute(raw, w - 2 * B, h - 2 * B, n, sort)


_REFS = {}


def reference(case_, oracle_lib):
    """Oracle outputs and intermediates of a case (test_gpu_fast_adversarial.build_ref) plus, per level,
    the raw keys, the budget and the definition's (result, Trace). Computed once per case, never modified."""
    if case_.name not in _REFS:
        from test_gpu_fast_adversarial import build_ref
        ref = build_ref(oracle_lib, case_.img, case_.nfeat, case_.scale, case_.nlevels, case_.ini, case_.min, case_.lap)
        ora = oracle_lib.OracleExtractor(case_.nfeat, case_.scale, case_.nlevels, case_.ini, case_.min)
        ref["budget"] = [int(v) for v in ora.level_info()["per_level"]]
        ora.close()
        sort = std_sort(oracle_lib)
        ref["raw"] = [[k for lst in ref["cells"][l][1] for k in lst] for l in range(case_.nlevels)]
        ref["levels"] = [run_definition(ref["raw"][l], ref["pyr"][l].shape[1], ref["pyr"][l].shape[0], ref["budget"][l], sort)
                         for l in range(case_.nlevels)]
        _REFS[case_.name] = ref
    return _REFS[case_.name]
