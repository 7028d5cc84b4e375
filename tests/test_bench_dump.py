"""bench.py --dump-outputs: the .npy files hold the front end's last-step outputs (what a caller of
StereoFrontEnd.run reads back), as float32 / float64, padding zeroed, for a seeded sample of frames."""
import os

import numpy as np
import pytest

import bench
from orb_slam3_ros_amd.synth import synth_stereo

EUROC_BF, EUROC_FX = 0.110078 * 458.654, 458.654


def test_dump_sample_is_fixed():
    a = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(512, 64, replace=False))
    b = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(512, 64, replace=False))
    assert np.array_equal(a, b) and len(set(a.tolist())) == 64
    # the sampled arrays of the default workload's capacity (about 1100 keypoints per image) fit the budget
    assert 64 * (2 * 1100 * (7 + 32) * 4 + 2 * 1100 * 4) <= bench.DUMP_BUDGET_BYTES < 64 << 20


@pytest.mark.gpu
def test_dump_outputs_match_front_end(gpu, tmp_path):
    import torch
    from orb_slam3_ros_amd.frontend import StereoFrontEnd
    F = 5
    pairs = [synth_stereo(700 + i, 752, 480) for i in range(F)]
    host = np.stack([img for p in pairs for img in p])
    images = torch.from_numpy(host).to(gpu)
    fe = StereoFrontEnd(F, 752, 480, nfeatures=1000, bf=EUROC_BF, fx=EUROC_FX, device=gpu)
    fe.run(images)
    out = tmp_path / "dump"
    bench.dump_outputs(fe, str(out))
    d = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(d) == {"sample_frames", "counts", "nmatch", "keypoints", "descriptors", "uright", "depth"}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    frames = d["sample_frames"].astype(int)
    assert frames.tolist() == list(range(F))   # F <= the sample size: every frame, ascending
    assert np.array_equal(d["counts"], fe.counts.cpu().numpy()) and d["counts"].shape == (2 * F, 2)
    assert np.array_equal(d["nmatch"], fe.nmatch.cpu().numpy()) and d["nmatch"].min() > 0
    for s, f in enumerate(frames):
        for side in (0, 1):
            mono, kp, desc = fe.host_image(2 * f + side)
            n, row = len(kp), 2 * s + side
            assert n == int(d["counts"][2 * f + side, 0]) > 900
            for c, name in enumerate(("x", "y", "size", "angle", "response", "octave", "class_id")):
                assert np.array_equal(d["keypoints"][row, :n, c], kp[name].astype(np.float32)), name
            assert np.array_equal(d["descriptors"][row, :n], desc.astype(np.float32))
            assert not d["keypoints"][row, n:].any() and not d["descriptors"][row, n:].any()
        kp, _, ur, dp = fe.host_frame(f)
        n = len(kp)
        assert np.array_equal(d["uright"][s, :n], ur) and np.array_equal(d["depth"][s, :n], dp)
        assert not d["uright"][s, n:].any() and not d["depth"][s, n:].any()
        assert int((ur >= 0).sum()) > 0
    fe.close()
