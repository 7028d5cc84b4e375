"""GPU parity of SearchByProjection on the planted cases of tests/sbp_patterns.py (each proved on the CPU
to reach the rule it names, tests/test_sbp_definition.py): every case through every form its variant has,
every slot and the return value equal to the C++ oracle's.

Which form runs is decided by sbp_run (orbfe_matcher.hip) from the shape alone, single camera:
  n <= 2048 keypoints and nq <= 2048 points        k_sbp_block<0 / 1 / 2>, one workgroup      "as planted"
  local map, n <= 2048, nq > 2048, th < 4          k_sbp_multi0 + k_sbp_multi                 queries padded, th 1, 3
  local map, n <= 2048, nq > 2048, th >= 4         k_sbp_band                                 queries padded, th 5
  local map, n > 2048, th < 2.5                    k_sbp_local                                keypoints padded, th 1
  local map, n > 2048, th >= 2.5                   k_sbp_local_wq<2>                          keypoints padded, th 3, 5
  last frame / keyframe, n > 2048 or nq > 2048     k_sbp_proj + k_mt_commit_count / _drop / _write
  device-resident local map, as planted            k_sbp_block<0> on the caller's arrays
Padding goes to 2,049, one past the limits, and is inert (sbp_patterns.pad_keys / pad_queries), so the
expected slots of a padded run are the planted run's. Every row of the table is asserted, not supposed:
the driver records the form it launched (orbfe_matcher_last_form, a host record that touches no kernel)
and each run must report the form of its row, so a moved threshold or a one-workgroup geometry that stops
fitting fails here instead of quietly testing another kernel. The counting mode (orbfe_matcher_set_stats)
is asserted as well: k_sbp_proj reports {0, 0, passes}, the one-workgroup and multi forms word 0 == word 1,
the pass forms pairs <= candidates. The bin plans also run through SearchForInitialization, whose
k_init_commit is the third copy of the histogram code.

The two-camera forms (k_sbp_block2, k_sbp_block4, k_sbp_local2, k_sbp_proj2) have their own planted cases in
tests/test_gpu_sbp_two_adversarial.py, SearchByBoW in tests/test_gpu_sbow_adversarial.py.
"""
import ctypes

import numpy as np
import pytest

import sbp_patterns as P
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.matcher import DeviceMatchFrame, ORBmatcher, search_by_projection_local_device

pytestmark = pytest.mark.gpu

CASES = P.all_cases()


@pytest.fixture(scope="module")
def counting(gpu):
    lib = _lib.load()
    lib.orbfe_matcher_set_stats(1)
    yield lib
    lib.orbfe_matcher_set_stats(0)


def _stats(lib):
    w = (ctypes.c_longlong * 3)()
    return lib.orbfe_matcher_last_stats(w), [int(x) for x in w]


def _run_gpu(case):
    mvp, p = case.mvp0.copy(), case.par
    m = ORBmatcher(p["nnratio"], p["check_ori"])
    if case.kind == "local":
        n = m.SearchByProjectionLocalMap(case.F, mvp, case.obs, case.q, p["th"])
    elif case.kind == "lastframe":
        n = m.SearchByProjectionLastFrame(case.F, mvp, case.obs, case.q, p["th"], p["fw"], p["bw"])
    else:
        n = m.SearchByProjectionKeyFrame(case.F, mvp, case.q, p["th"], p["ORBdist"])
    return n, mvp


# orbfe_matcher_last_form (include/orbfe.h)
FORM_BLOCK, FORM_MULTI, FORM_BAND, FORM_LOCAL, FORM_LOCAL_WQ2, FORM_PROJ = 1, 2, 3, 4, 7, 8


def _form(case, padded):
    """The form sbp_run picks for the shape (the table in the module docstring) and its counting kind."""
    if padded is None:
        return FORM_BLOCK, "same"
    if case.kind != "local":
        return FORM_PROJ, "proj"
    if padded == "queries":
        return (FORM_MULTI, "same") if case.par["th"] < 4 else (FORM_BAND, "pass")
    return (FORM_LOCAL, "pass") if case.par["th"] < 2.5 else (FORM_LOCAL_WQ2, "pass")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_every_form(counting, oracle_lib, case):
    n_o, mvp_o = P.run_oracle(oracle_lib, case)
    for padded in (None, "queries", "keys"):
        c = case if padded is None else P.pad_queries(case) if padded == "queries" else P.pad_keys(case)
        assert (c.F.N > 2048) == (padded == "keys") and (len(c.q) > 2048) == (padded == "queries")
        form, kind = _form(case, padded)
        n, mvp = _run_gpu(c)
        rc, w = _stats(counting)
        assert counting.orbfe_matcher_last_form() == form, (padded, counting.orbfe_matcher_last_form(), form)
        assert n == n_o, (form, n, n_o)
        np.testing.assert_array_equal(mvp[:case.F.N], mvp_o, err_msg=form)
        assert (mvp[case.F.N:] == -1).all(), form
        assert rc == _lib.ORBFE_OK and w[2] >= 1, (form, rc, w)
        if kind == "proj":
            assert w[:2] == [0, 0], (form, w)
        elif kind == "same":
            assert w[0] == w[1], (form, w)
        else:
            assert w[1] <= w[0], (form, w)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "local"], ids=repr)
def test_local_device_resident(counting, gpu, oracle_lib, case):
    import torch
    n_o, mvp_o = P.run_oracle(oracle_lib, case)
    Fd = DeviceMatchFrame(case.F, gpu)
    mvp = torch.from_numpy(case.mvp0.copy()).to(gpu)
    obs = torch.from_numpy(case.obs.copy()).to(gpu)
    mps = torch.from_numpy(case.q.view(np.uint8).reshape(-1).copy()).to(gpu)
    n = search_by_projection_local_device(Fd, mvp, obs, mps, case.par["th"], nnratio=case.par["nnratio"])
    assert counting.orbfe_matcher_last_form() == FORM_BLOCK
    assert n == n_o
    np.testing.assert_array_equal(mvp.cpu().numpy(), mvp_o)


@pytest.mark.parametrize("case", P.init_cases(), ids=repr)
def test_init_bin_plans(gpu, oracle_lib, case):
    pa, pb = case.prev(), case.prev()
    ma = np.zeros(case.F1.N, np.int32)
    mb = np.zeros(case.F1.N, np.int32)
    na = oracle_lib.OracleMatcher(0.9, True).search_for_init(case.F1, case.F2, pa, ma, 10)
    nb = ORBmatcher(0.9, True).SearchForInitialization(case.F1, case.F2, pb, mb, 10)
    assert na == nb == int((case.expect >= 0).sum())
    np.testing.assert_array_equal(mb, ma)
    np.testing.assert_array_equal(mb, case.expect)
    np.testing.assert_array_equal(pb, pa)
