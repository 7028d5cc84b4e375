"""CPU: the definitional DistributeOctTree (oracle/octree_definition.py) against the C++ oracle on
every adversarial case of tests/octree_patterns.py, and every case's precondition.

For every case and level the oracle's raw keys (vToDistributeKeys order) go through the definition
with the level's budget; the result must equal the oracle's octree output in x, y and score, in list
order. Level 0's raw keys are also the definitional FAST's (oracle/fast_definition.py), so the
planted key sets are confirmed. Each case's pre() then asserts, from the definition's trace alone,
that the case reaches the k_octree branch it is named for; tests/test_gpu_octree_adversarial.py
relies on that. One 752 x 480, 1000-feature, 8-level synthetic frame ties the definition to the
workload geometry.
"""
import numpy as np
import pytest

import octree_patterns as op
from oracle import fast_definition as fd

CASES = op.all_cases()


def oracle_octree(ref, level):
    o = ref["oct"][level]
    return list(zip((o["x"] - op.B).astype(int).tolist(), (o["y"] - op.B).astype(int).tolist(),
                    o["response"].astype(int).tolist()))


def check_definition(ref, nlevels, what):
    for l in range(nlevels):
        out, tr = ref["levels"][l]
        want = oracle_octree(ref, l)
        assert tr.K == len(ref["raw"][l])
        assert len(out) == len(want), f"{what} level {l}: definition {len(out)} keys, oracle {len(want)}"
        bad = [i for i, (a, b) in enumerate(zip(out, want)) if a != b]
        assert not bad, f"{what} level {l}: {len(bad)} keys differ, first at {bad[0]}: {out[bad[0]]} vs {want[bad[0]]}"


def test_case_names_unique():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_definition_equals_oracle(case, oracle_lib):
    ref = op.reference(case, oracle_lib)
    # the level-0 keys the octree gets are the definitional FAST's, in the same order
    lists = fd.cell_keys(case.img, case.ini, case.min)[1]
    assert ref["raw"][0] == [k for l in lists for k in l]
    check_definition(ref, case.nlevels, case.name)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_precondition(case, oracle_lib):
    case.pre(case, op.reference(case, oracle_lib)["levels"])


def test_thread_counts_covered(oracle_lib):
    """Over all cases, both instances take every step form, key storage, finish reason and rank pass
    they have."""
    seen = {nt: set() for nt in (op.NT_BATCH, op.NT_HOST)}
    for c in CASES:
        for nt in seen:
            seen[nt] |= op.branches(op.reference(c, oracle_lib)["levels"], nt)
    common = {"p1-fused", "p1-generic", "p2-fused", "p2-generic-m", "p2-generic-n", "finish-p1-reach-N", "finish-p2-reach-N",
              "finish-stall-cluster", "finish-stall-singles", "ranks-one-scan", "ranks-two-scans", "keys-in-global-lists",
              "roots-scanned"}
    assert common <= seen[op.NT_BATCH], sorted(common - seen[op.NT_BATCH])
    want_host = common | {"keys-in-registers", "roots-per-thread"}
    assert want_host <= seen[op.NT_HOST], sorted(want_host - seen[op.NT_HOST])


def test_workload_geometry(oracle_lib):
    """A 752 x 480 synthetic frame at 1000 features, 8 levels: the bench geometry."""
    from orb_slam3_ros_amd import synth
    img = synth.synth_image(5, 752, 480)
    case = op.case("workload-752x480", img, 1000, None, nlevels=8)
    ref = op.reference(case, oracle_lib)
    check_definition(ref, 8, case.name)
    assert sum(len(out) for out, _ in ref["levels"]) == len(ref["kp"]) > 900
    assert {tr.n_ini for _, tr in ref["levels"]} == {2}
