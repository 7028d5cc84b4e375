"""CPU: the C surface of the batched SearchForTriangulation. The argument checks and trivial returns of
orbfe_search_for_triangulation_batch run before any device call, so they answer on a machine without a
GPU. A resident handle cannot be made here; the refusals that need one (no geometry, a repeated index, a
two-camera keyframe without bCoarse) are in tests/test_gpu_tri_batch.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from orb_slam3_ros_amd import _lib

OK, E_ARG = _lib.ORBFE_OK, _lib.ORBFE_E_ARG
NEW = ("orbfe_keyframe_create_geom", "orbfe_keyframe_has_geom", "orbfe_search_for_triangulation_batch",
       "orbfe_matcher_last_tri_batch")


def test_symbols_are_exported_and_bound(orbfe_lib):
    for name in NEW:
        assert name in _lib._SIGS
        fn = getattr(orbfe_lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(_lib._SIGS[name][1])
    from orb_slam3_ros_amd.matcher import KeyFrameFeatures, ORBmatcher, TriJob
    assert callable(ORBmatcher.SearchForTriangulationBatch) and callable(ORBmatcher.last_tri_batch)
    assert isinstance(KeyFrameFeatures.has_geom, property) and callable(TriJob.make)


def test_tri_job_layout_matches_header(tmp_path):
    """struct orbfe_tri_job as the C compiler lays it out (include/orbfe.h) == the ctypes mirror."""
    from orb_slam3_ros_amd.matcher import TriJob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("gcc") or shutil.which("cc")
    cmd = [cc] if cc else ["g++", "-x", "c"]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbfe.h"\nint main(void){printf("%zu %zu %zu %zu",'
                   ' sizeof(orbfe_tri_job), offsetof(orbfe_tri_job, mp2), offsetof(orbfe_tri_job, F12),'
                   ' offsetof(orbfe_tri_job, ep));return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.run(cmd + ["-I", os.path.join(root, "include"), "-o", str(exe), str(src)], check=True)
    got = tuple(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == (ctypes.sizeof(TriJob), TriJob.mp2.offset, TriJob.F12.offset, TriJob.ep.offset)
    assert got[0] == 64   # two pointers, 11 floats, padding


def test_trivial_returns_and_refusals(orbfe_lib):
    from orb_slam3_ros_amd.matcher import TriJob
    call = orbfe_lib.orbfe_search_for_triangulation_batch
    out, nm = np.full(8, 7, np.int32), np.full(2, 7, np.int32)
    mp1 = np.zeros(8, np.int32)
    jobs = (TriJob * 2)()
    o, n = out.ctypes.data, nm.ctypes.data
    # no jobs: nothing to do, whatever the other arguments are
    assert call(None, None, None, 0, 0, 0, 1, o, n) == OK
    assert call(None, None, None, -1, 0, 0, 1, o, n) == E_ARG
    # NULL outputs (the handle argument is never dereferenced: the check comes first)
    assert call(1, mp1.ctypes.data, jobs, 2, 0, 0, 1, None, n) == E_ARG
    assert call(1, mp1.ctypes.data, jobs, 2, 0, 0, 1, o, None) == E_ARG
    assert call(1, mp1.ctypes.data, jobs, 0, 0, 0, 1, None, None) == E_ARG
    # NULL current keyframe, NULL job table
    assert call(None, mp1.ctypes.data, jobs, 2, 0, 0, 1, o, n) == E_ARG
    assert call(None, mp1.ctypes.data, None, 2, 0, 0, 1, o, n) == E_ARG
    assert (out == 7).all() and (nm == 7).all()   # a refusal writes nothing
    # the create's refusals that come before its first device call
    h = ctypes.c_void_p(5)
    assert orbfe_lib.orbfe_keyframe_create_geom(None, None, None, ctypes.byref(h)) == E_ARG and h.value is None
    assert orbfe_lib.orbfe_keyframe_create_geom(None, None, None, None) == E_ARG
    assert orbfe_lib.orbfe_keyframe_has_geom(None) == E_ARG


def test_create_geom_refusals_need_no_device(orbfe_lib):
    """nlevels < 1, a NULL scale_factors or level_sigma2, an octave outside [0, nlevels): ORBFE_E_ARG before
    any allocation, so without a device."""
    from orb_slam3_ros_amd import synth_match as sm
    from orb_slam3_ros_amd.matcher import CFrame, FeatureVector
    rng = np.random.default_rng(3)
    F = sm.synth_frame(rng, 40, stereo=True)
    fv = FeatureVector({3: list(range(20)), 9: list(range(20, 40))})
    sg = (F.scale_factors * F.scale_factors).astype(np.float32)

    def create(edit, sigma2=sg):
        c = CFrame()
        ctypes.memmove(ctypes.byref(c), F.ref(), ctypes.sizeof(CFrame))
        keep = edit(c)
        h = ctypes.c_void_p(5)
        rc = orbfe_lib.orbfe_keyframe_create_geom(ctypes.byref(c), fv.ref(), None if sigma2 is None else sigma2.ctypes.data,
                                                  ctypes.byref(h))
        assert h.value is None
        return rc, keep

    def no_levels(c):
        c.nlevels = 0

    def no_scales(c):
        c.scale_factors = None

    def bad_octave(c, octave):
        k = F.keys.copy()
        k["octave"][17] = octave
        c.keys = k.ctypes.data
        return k
    assert create(no_levels)[0] == E_ARG
    assert create(no_scales)[0] == E_ARG
    assert create(lambda c: None, sigma2=None)[0] == E_ARG
    assert create(lambda c: bad_octave(c, 8))[0] == E_ARG
    assert create(lambda c: bad_octave(c, -1))[0] == E_ARG


def test_last_form_record(orbfe_lib):
    w = np.full(3, 7, np.int32)
    assert orbfe_lib.orbfe_matcher_last_tri_batch(None) == E_ARG
    out, nm = np.full(8, 7, np.int32), np.full(2, 7, np.int32)
    assert orbfe_lib.orbfe_search_for_triangulation_batch(None, None, None, -1, 0, 0, 1, out.ctypes.data,
                                                          nm.ctypes.data) == E_ARG
    assert orbfe_lib.orbfe_matcher_last_tri_batch(w.ctypes.data) == OK
    assert w.tolist() == [0, 0, 0]   # a refused call ran no form
