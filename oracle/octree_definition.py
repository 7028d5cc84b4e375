"""DistributeOctTree written from its description, in plain Python — TEST INFRASTRUCTURE ONLY.

An independent second reference for the key distribution: when the HIP kernel and the C++ oracle
disagree on a level's keys, this module says which side is wrong. It touches no GPU and no C++;
the one thing it borrows is the phase-2 sort, passed in as a callable, because the answer depends
on the tie order of the host's std::sort (tests pass the oracle's exported libstdc++ sort, which
tests/test_native_checks.py pins).

Algorithm ("Octree"; oracle/orb_oracle.cpp distribute_octtree). The detection area of a
level, width x height, is cut into nIni = round(width / height) root columns of fractional width
hX = width / nIni (float): root i spans x in [(int)(hX i), (int)(hX (i + 1))), and a key belongs
to root (int)(x / hX). Empty roots are dropped. A node with one key is final. A round divides
every node with more than one key into four children (x split at ceil(w / 2), y at ceil(h / 2)),
pushes the non-empty children to the front of the node list in the order n1, n2, n3, n4 (so n4
ends up first) and erases the parent. Rounds over the whole list in list order are phase 1. When
the list, after a phase-1 round, holds n nodes of which m have several keys and n + 3 m > N, phase 2
takes over: the m expandable nodes, in the order they were pushed, are sorted by (size, UL.x)
ascending and divided from the back, stopping the moment the list reaches N. Either phase ends the
whole distribution when the list reaches N nodes or a round leaves its length unchanged (the stall
rule: a tight cluster whose node keeps one non-empty child). Each remaining node yields its key of
maximal score, the first in key order among equals.

Every value the reference holds in a `float` is an np.float32 here: hX, x / hX, hX * i.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F32 = np.float32


@dataclass(eq=False)
class Node:
    x0: int
    x1: int
    y0: int
    y1: int
    keys: list = field(default_factory=list)   # (x, y, score, index in the input order)
    final: bool = False


@dataclass
class Round:
    phase: int        # 1 or 2
    n: int            # nodes in the list after the round
    m: int            # of the nodes pushed in the round, those with several keys
    divided: int      # nodes divided in the round
    finish: str | None = None   # None, "reach-N" or "stall"
    # phase 2 only
    sorted_m: int = 0           # entries sorted
    tie_group: bool = False     # two sorted entries with equal (size, UL.x)
    break_at: int | None = None   # walk position t (0 = largest node) whose division reached N
    break_in_tie: bool = False  # the entry after the break (not divided) ties with the last divided one


@dataclass
class Trace:
    K: int = 0
    N: int = 0
    n_ini: int = 0
    hx: float = 0.0
    empty_roots: int = 0
    roots: int = 0                   # nodes in the initial list
    rounds: list = field(default_factory=list)
    boundary_keys: list = field(default_factory=list)   # (x, i): x == (int)(hX (i + 1)), i + 1 < nIni
    score_tie_nodes: int = 0         # final nodes holding several keys of maximal score
    finish: str = ""                 # finish reason of the last round


def _round_half_away(v) -> int:
    v = float(v)
    return int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))


def root_geometry(width: int, height: int):
    """(nIni, hX as float32, [(x0, x1)] of every root column)."""
    n_ini = _round_half_away(F32(width) / F32(height))
    hx = F32(width) / F32(n_ini)
    return n_ini, hx, [(int(hx * F32(i)), int(hx * F32(i + 1))) for i in range(n_ini)]


def root_of(x: int, hx) -> int:
    return int(F32(x) / hx)


def _divide(nd: Node):
    hx, hy = -(-(nd.x1 - nd.x0) // 2), -(-(nd.y1 - nd.y0) // 2)
    mx, my = nd.x0 + hx, nd.y0 + hy
    ch = [Node(nd.x0, mx, nd.y0, my), Node(mx, nd.x1, nd.y0, my), Node(nd.x0, mx, my, nd.y1), Node(mx, nd.x1, my, nd.y1)]
    for k in nd.keys:
        ch[(0 if k[0] < mx else 1) + (0 if k[1] < my else 2)].keys.append(k)
    for c in ch:
        c.final = len(c.keys) == 1
    return ch


def distribute(keys, width: int, height: int, N: int, sort):
    """keys: [(x, y, score)] in vToDistributeKeys order, coordinates relative to the level's border;
    width, height: the detection area (maxBorder - minBorder); sort(list of u64) -> the list sorted
    by the high 32 bits as std::sort with compareNodes orders it. Returns (result keys in node-list
    order as [(x, y, score)], Trace)."""
    tr = Trace(K=len(keys), N=N)
    n_ini, hx, cols = root_geometry(width, height)
    tr.n_ini, tr.hx = n_ini, float(hx)
    roots = [Node(x0, x1, 0, height) for x0, x1 in cols]
    for idx, (x, y, s) in enumerate(keys):
        roots[root_of(x, hx)].keys.append((int(x), int(y), int(s), idx))
        for i in range(n_ini - 1):
            if int(x) == cols[i][1]:
                tr.boundary_keys.append((int(x), i))
    nodes = []
    for r in roots:
        if not r.keys:
            tr.empty_roots += 1
            continue
        r.final = len(r.keys) == 1
        nodes.append(r)
    tr.roots = len(nodes)

    pushed = []   # nodes with several keys, in push order (vSizeAndPointerToNode)

    def push_children(ch):
        added = 0
        for c in ch:
            if c.keys:
                nodes.insert(0, c)
                added += 1
                if len(c.keys) > 1:
                    pushed.append(c)
        return added

    finish = None
    while finish is None:
        prev = len(nodes)
        pushed.clear()
        i, divided = 0, 0
        while i < len(nodes):
            nd = nodes[i]
            if nd.final:
                i += 1
                continue
            i += push_children(_divide(nd))
            del nodes[i]
            divided += 1
        rd = Round(1, len(nodes), len(pushed), divided)
        tr.rounds.append(rd)
        if len(nodes) >= N:
            finish = "reach-N"
        elif len(nodes) == prev:
            finish = "stall"
        rd.finish = finish
        if finish is None and len(nodes) + 3 * len(pushed) > N:
            while finish is None:
                prev = len(nodes)
                vprev = list(pushed)
                pushed.clear()
                packed = [(((len(nd.keys) << 12) | nd.x0) << 32) | j for j, nd in enumerate(vprev)]
                order = [int(v) for v in sort(packed)]
                hi = [v >> 32 for v in order]
                assert hi == sorted(hi), "sort() did not sort by the high word"
                rd = Round(2, 0, 0, 0, sorted_m=len(order))
                rd.tie_group = any(a == b for a, b in zip(hi, hi[1:]))
                for j in range(len(order) - 1, -1, -1):
                    nd = vprev[order[j] & 0xffffffff]
                    push_children(_divide(nd))
                    nodes.remove(nd)
                    rd.divided += 1
                    if len(nodes) >= N:
                        rd.break_at = len(order) - 1 - j
                        rd.break_in_tie = j > 0 and hi[j - 1] == hi[j]
                        break
                rd.n, rd.m = len(nodes), len(pushed)
                tr.rounds.append(rd)
                if len(nodes) >= N:
                    finish = "reach-N"
                elif len(nodes) == prev:
                    finish = "stall"
                rd.finish = finish
    tr.finish = finish
    out = []
    for nd in nodes:
        best = nd.keys[0]
        for k in nd.keys[1:]:
            if k[2] > best[2]:
                best = k
        if sum(1 for k in nd.keys if k[2] == best[2]) > 1:
            tr.score_tie_nodes += 1
        out.append(best[:3])
    return out, tr
