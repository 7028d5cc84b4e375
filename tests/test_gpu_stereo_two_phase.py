"""GPU parity of the two-phase k_stereo (match all keys and compact the ones that reach the window search,
then the SAD refinement over the compacted list with the next items' rows loaded ahead) on the planted
cases of tests/stereo_two_phase_patterns.py, bit-exact against the CPU oracle in both launch forms of
orbfe_stereo_match_batch. The harness is the one of tests/test_gpu_stereo_adversarial.py: planted
records on extracted pyramids, uRight and depth compared as bit patterns, the match count, sentinels
past every frame's N and a guard frame.

  work list    0, 1, 2, 3, 5 and 65 entries: an empty phase B, idle lane groups, the odd tail, and the
               rows loaded ahead past the end of the list (one more than a wave iteration's 4 items and
               than a block round's 64)
  bounds test  every match rejected by iniu < 0 (empty list, every output -1), and such keys between
               true matches (list index != key index)
  ties         equal best distances in a band of 74 candidates, the lower right index met in an
               earlier and in a later scan trip
  counts       N = 0, Nr = 0, N = 512 + 3 (a second block of three keys)
  levels       neighbouring list items on different levels, level 0 read from caller images with an odd
               pitch and base offset
"""
import numpy as np
import pytest

import stereo_patterns as sp
import stereo_two_phase_patterns as tp
from test_gpu_stereo_adversarial import SMALL_BATCH, Rig, run_frames

pytestmark = pytest.mark.gpu

CASES = tp.all_cases()


@pytest.fixture(scope="module")
def refs(oracle_lib):
    """Oracle reference and asserted precondition of every case, once for the module."""
    out = {}
    for c in CASES:
        sp.validate(c, sp.CAP[c.g])
        ref = sp.reference(c, oracle_lib)
        sp.check_windows(c, ref["def"][3])
        c.pre(c, ref)   # CPU: the case reaches its branch
        out[c.name] = ref["oracle"]
    return out


@pytest.fixture(scope="module")
def rig(gpu):
    r = Rig(gpu)
    yield r
    r.close()


@pytest.mark.parametrize("two_handles", [True, False], ids=["two-handles", "one-handle-stride-2"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_small_batch(case, two_handles, rig, refs):
    """One frame: fewer than 16, so 16 left keys per block."""
    frames = [case]
    assert len(frames) < SMALL_BATCH
    run_frames(rig, frames, refs, two_handles, "two-phase-small")


def _groups():
    by = {}
    for c in CASES:
        by.setdefault((c.pair, c.layout, c.bf, c.fx), []).append(c)
    out = []
    for cs in by.values():
        for i in range(0, len(cs), SMALL_BATCH - 2):
            out.append(cs[i:i + SMALL_BATCH - 2])
    return out


@pytest.mark.parametrize("group", _groups(), ids=lambda g: "+".join(c.name for c in g))
def test_large_batch(group, rig, refs, oracle_lib):
    """16 frames in one batch of 32 images (512 left keys per block), the cases in shuffled slots, the
    spare slots filled with frames that have N = 0 or Nr = 0."""
    c0 = group[0]
    fill = []
    for k in range(SMALL_BATCH - len(group)):   # at least two: N = 0 and Nr = 0
        f = sp.fillers(c0.pair)[k % 2]
        f.layout, f.bf, f.fx = c0.layout, c0.bf, c0.fx
        f.name += f"-two-phase-{k}"
        sp.validate(f, sp.CAP[f.g])
        refs[f.name] = sp.reference(f, oracle_lib)["oracle"]
        fill.append(f)
    frames = group + fill
    order = np.random.default_rng(7100 + len(group)).permutation(len(frames))
    frames = [frames[i] for i in order]
    assert len(frames) == SMALL_BATCH and not len(frames) < SMALL_BATCH
    assert [f.name for f in frames] != [f.name for f in group + fill]
    run_frames(rig, frames, refs, False, "two-phase-large")
