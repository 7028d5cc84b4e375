"""CPU: the C surface of the batched Fuse. The argument checks and trivial returns of orbfe_fuse_batch and
the refusals of orbfe_keyframe_create_grid run before any device call, so they answer on a machine without
a GPU. A resident handle cannot be made here; the refusals that need one (a handle without a grid, bRight
on a single-camera keyframe) are in tests/test_gpu_fuse_batch.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

from orb_slam3_ros_amd import _lib

OK, E_ARG = _lib.ORBFE_OK, _lib.ORBFE_E_ARG
NEW = ("orbfe_keyframe_create_grid", "orbfe_keyframe_has_grid", "orbfe_fuse_batch", "orbfe_matcher_last_fuse_batch")


def test_symbols_are_exported_and_bound(orbfe_lib):
    for name in NEW:
        assert name in _lib._SIGS
        fn = getattr(orbfe_lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(_lib._SIGS[name][1])
    from orb_slam3_ros_amd.matcher import FuseJob, KeyFrameFeatures, ORBmatcher
    assert callable(ORBmatcher.FuseBatch) and callable(ORBmatcher.last_fuse_batch)
    assert callable(KeyFrameFeatures.has_grid) and callable(FuseJob.make)


def test_fuse_job_layout_matches_header(tmp_path):
    """struct orbfe_fuse_job as the C compiler lays it out (include/orbfe.h) == the ctypes mirror."""
    from orb_slam3_ros_amd.matcher import FuseJob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("gcc") or shutil.which("cc")
    cmd = [cc] if cc else ["g++", "-x", "c"]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbfe.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu",'
                   ' sizeof(orbfe_fuse_job), offsetof(orbfe_fuse_job, kf), offsetof(orbfe_fuse_job, skip),'
                   ' offsetof(orbfe_fuse_job, cam), offsetof(orbfe_fuse_job, model), offsetof(orbfe_fuse_job, bRight));'
                   'return 0;}\n')
    exe = tmp_path / "lay"
    subprocess.run(cmd + ["-I", os.path.join(root, "include"), "-o", str(exe), str(src)], check=True)
    got = tuple(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == (ctypes.sizeof(FuseJob), FuseJob.kf.offset, FuseJob.skip.offset, FuseJob.cam.offset,
                   FuseJob.model.offset, FuseJob.bRight.offset)
    assert got[0] == 120   # two pointers, a 64-byte camera, a 36-byte model, bRight


def test_trivial_returns_and_refusals(orbfe_lib):
    """n_jobs == 0 is ORBFE_OK whatever else is passed; every refusal that needs no handle is ORBFE_E_ARG
    and leaves the three output arrays as they were. The jobs hold NULL handles, which are never
    dereferenced."""
    from orb_slam3_ros_amd.matcher import MAP_POINT_3D_DTYPE, FuseJob
    call = orbfe_lib.orbfe_fuse_batch
    n = 5
    bi, bd, nf = np.full(2 * n, 7, np.int32), np.full(2 * n, 7, np.int32), np.full(2, 7, np.int32)
    pts = np.zeros(n, MAP_POINT_3D_DTYPE)
    jobs = (FuseJob * 2)()
    P, I, D, N = pts.ctypes.data, bi.ctypes.data, bd.ctypes.data, nf.ctypes.data
    for sim3 in (0, 1):
        # no jobs: nothing to do, whatever the other arguments are
        assert call(None, 0, None, 0, 3.0, sim3, None, None, None) == OK
        assert call(jobs, 0, P, n, 3.0, sim3, I, D, N) == OK
        # negative counts
        assert call(jobs, -1, P, n, 3.0, sim3, I, D, N) == E_ARG
        assert call(jobs, 2, P, -1, 3.0, sim3, I, D, N) == E_ARG
        assert call(None, -1, None, -1, 3.0, sim3, None, None, None) == E_ARG
        # each NULL array where the call needs it
        assert call(None, 2, P, n, 3.0, sim3, I, D, N) == E_ARG
        assert call(jobs, 2, None, n, 3.0, sim3, I, D, N) == E_ARG
        assert call(jobs, 2, P, n, 3.0, sim3, None, D, N) == E_ARG
        assert call(jobs, 2, P, n, 3.0, sim3, I, None, N) == E_ARG
        assert call(jobs, 2, P, n, 3.0, sim3, I, D, None) == E_ARG
        assert call(jobs, 2, None, 0, 3.0, sim3, None, None, None) == E_ARG   # nfused is needed without points too
        assert (bi == 7).all() and (bd == 7).all() and (nf == 7).all()   # a refusal writes nothing
    # the create's refusals that come before its first device call
    h = ctypes.c_void_p(5)
    assert orbfe_lib.orbfe_keyframe_create_grid(None, None, None, ctypes.byref(h)) == E_ARG and h.value is None
    assert orbfe_lib.orbfe_keyframe_create_grid(None, None, None, None) == E_ARG
    assert orbfe_lib.orbfe_keyframe_has_grid(None) == E_ARG


def test_rows_without_a_live_job_need_no_device(orbfe_lib):
    """Jobs with NULL handles only (isBad() keyframes), and a call without points: every row is -1 and every
    nfused 0, written on the host."""
    from orb_slam3_ros_amd.matcher import MAP_POINT_3D_DTYPE, FuseJob
    n = 5
    bi, bd, nf = np.full(2 * n, 7, np.int32), np.full(2 * n, 7, np.int32), np.full(2, 7, np.int32)
    pts = np.zeros(n, MAP_POINT_3D_DTYPE)
    jobs = (FuseJob * 2)()
    w = np.zeros(3, np.int32)
    assert orbfe_lib.orbfe_fuse_batch(jobs, 2, pts.ctypes.data, n, 3.0, 0, bi.ctypes.data, bd.ctypes.data,
                                      nf.ctypes.data) == OK
    assert (bi == -1).all() and (bd == -1).all() and (nf == 0).all()
    assert orbfe_lib.orbfe_matcher_last_fuse_batch(w.ctypes.data) == OK and w.tolist() == [0, 2, 0]
    nf[:] = 7
    assert orbfe_lib.orbfe_fuse_batch(jobs, 2, None, 0, 4.0, 1, None, None, nf.ctypes.data) == OK
    assert (nf == 0).all()


def test_create_grid_refusals_need_no_device(orbfe_lib):
    """What orbfe_keyframe_create_geom refuses, empty bounds, more than 8,192 keypoints and a two-camera
    keyframe whose nleft lies outside [0, n]: ORBFE_E_ARG before any allocation, so without a device."""
    from orb_slam3_ros_amd import synth_match as sm
    from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
    from orb_slam3_ros_amd.matcher import CFrame, FeatureVector
    rng = np.random.default_rng(3)
    F = sm.synth_frame(rng, 40, stereo=True)
    fv = FeatureVector({3: list(range(20)), 9: list(range(20, 40))})
    sg = (F.scale_factors * F.scale_factors).astype(np.float32)

    def create(edit, sigma2=sg, featvec=fv):
        c = CFrame()
        ctypes.memmove(ctypes.byref(c), F.ref(), ctypes.sizeof(CFrame))
        keep = edit(c)
        h = ctypes.c_void_p(5)
        rc = orbfe_lib.orbfe_keyframe_create_grid(ctypes.byref(c), featvec.ref(), None if sigma2 is None else sigma2.ctypes.data,
                                                  ctypes.byref(h))
        assert h.value is None
        return rc, keep

    def field(name, value):
        def edit(c):
            setattr(c, name, value)
        return edit

    def bad_octave(c):
        k = F.keys.copy()
        k["octave"][17] = 8
        c.keys = k.ctypes.data
        return k

    def too_many(c):
        k = np.zeros(8193, KEYPOINT_DTYPE)
        d = np.zeros((8193, 32), np.uint8)
        c.n, c.keys, c.desc, c.uright = 8193, k.ctypes.data, d.ctypes.data, None
        return k, d

    def two(nleft):
        def edit(c):
            c.two_cams, c.nleft = 1, nleft
        return edit
    # what the geometry create refuses
    assert create(field("nlevels", 0))[0] == E_ARG
    assert create(field("scale_factors", None))[0] == E_ARG
    assert create(lambda c: None, sigma2=None)[0] == E_ARG
    assert create(bad_octave)[0] == E_ARG
    # the grid's own
    assert create(field("max_x", F.c.min_x))[0] == E_ARG
    assert create(field("max_y", F.c.min_y - 1.0))[0] == E_ARG
    assert create(too_many, featvec=FeatureVector({}))[0] == E_ARG
    assert create(two(-1))[0] == E_ARG
    assert create(two(41))[0] == E_ARG


def test_last_form_record(orbfe_lib):
    w = np.full(3, 7, np.int32)
    assert orbfe_lib.orbfe_matcher_last_fuse_batch(None) == E_ARG
    nf = np.full(2, 7, np.int32)
    assert orbfe_lib.orbfe_fuse_batch(None, -1, None, 0, 3.0, 0, None, None, nf.ctypes.data) == E_ARG
    assert orbfe_lib.orbfe_matcher_last_fuse_batch(w.ctypes.data) == OK
    assert w.tolist() == [0, 0, 0]   # a refused call ran no form
