"""GPU parity of SearchForInitialization on the planted cases of tests/init_patterns.py (each proved on the
CPU to reach the rule it names, tests/test_init_definition.py): the return value, vnMatches12 and
vbPrevMatched equal the definition's (oracle/init_definition.py), exactly: every quantity is an integer or a
copied float.

  k_init_state   the per-candidate selector segments (512 selectors of one key, in four distance orders)
  k_init_eval    window cells and early returns, the strict box, 16-lane column walk (1 to 35 columns, best and
                 second best in one lane and in two), blocked candidates and bestDist2, the level filter and
                 the unfiltered negative-octave queries, partly filled waves (n1 = 1 .. 65)
  k_init_commit  steals, the votes of stolen selections, the three-maxima cut at 0.1f * max1
  host           the level-0 subsets and their scatter, empty subsets, the whole-frame path (negative octaves),
                 more than one round trip of gated passes (chain-12: 14 passes, chain-25: 27), the 8192 limit

Every case runs twice on one matcher with another case in between (stale arena, change-flag or status
state would show in the second run).
"""
import numpy as np
import pytest

import init_patterns as P
from orb_slam3_ros_amd._lib import OrbfeCapacityError, OrbfeError
from orb_slam3_ros_amd.matcher import ORBmatcher

pytestmark = pytest.mark.gpu

CASES = P.all_cases()


@pytest.fixture(scope="module")
def expected():
    """The definition's (n, vnMatches12, vbPrevMatched) of every case, computed once."""
    return {c.name: P.run_definition(c)[:3] for c in CASES}


def _run(case):
    prev, m12 = case.prev.copy(), np.full(case.F1.N, -7, np.int32)
    n = ORBmatcher(case.nnratio, case.check_ori).SearchForInitialization(case.F1, case.F2, prev, m12, case.window)
    return n, m12, prev


def _assert_equal(got, want, name):
    assert got[0] == want[0], (name, got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1], err_msg=name)
    np.testing.assert_array_equal(got[2], want[2], err_msg=name)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c.name for c in CASES])
def test_case(gpu, expected, k):
    case, other = CASES[k], CASES[(k + 7) % len(CASES)]
    _assert_equal(_run(case), expected[case.name], case.name)
    _assert_equal(_run(other), expected[other.name], other.name)
    _assert_equal(_run(case), expected[case.name], case.name + " (second run)")


def test_lattice_full_capacity(gpu):
    """n1 = n2 = 8192, the largest frames the matcher takes, every key at level 0."""
    case = P.lattice_case()
    want = P.run_definition(case)[:3]
    assert want[0] > P.MAX_N // 4
    _assert_equal(_run(case), want, case.name)
    _assert_equal(_run(CASES[0]), P.run_definition(CASES[0])[:3], CASES[0].name)
    _assert_equal(_run(case), want, case.name + " (second run)")


@pytest.mark.parametrize("side", [1, 2])
def test_one_past_capacity_is_an_argument_error(gpu, side):
    big, small = P.lattice_case(P.MAX_N + 1), CASES[0]
    F1, F2, prev = (big.F1, small.F2, big.prev) if side == 1 else (small.F1, big.F2, small.prev)
    assert max(F1.N, F2.N) == P.MAX_N + 1
    m12 = np.full(F1.N, -7, np.int32)
    with pytest.raises(OrbfeError, match="bad argument") as e:
        ORBmatcher(0.9, True).SearchForInitialization(F1, F2, prev.copy(), m12, 6)
    assert not isinstance(e.value, OrbfeCapacityError)
    assert (m12 == -7).all()   # refused before anything is written
