"""GPU: a matcher call's answer does not depend on what earlier calls of the thread left in the arena.

Every matcher entry carves its scratch out of one per-thread device arena, one mapped pinned staging block and
one mapped slot block, none of which is ever cleared; only selected words are zeroed per call. The adversarial
suites run a case at a time against the oracle, which checks the arithmetic. Here the same planted cases (nothing
new is planted: the first case of every kind each pattern module defines) run with the arena under the test's
control: filled with a 32-bit word by orbfe_debug_fill_matcher between two runs, after a sibling of the same
shape and other content, interleaved across families in a shuffled order, with the pass hint of a many-pass
search in front of a one-pass search, and with device-resident searches on two streams around a host call.
Expected values are the oracle's, as in the adversarial suites, whose runners and form assertions
(orbfe_matcher_last_form and its kin) are used as they are.

Fill words are 0 and 1 only: read as a count, an index, a flag or a float, both stay inside every array, so a
stale read gives a wrong answer and never a wild address; a predecessor has the array sizes of the call under
test for the same reason."""
import ctypes

import numpy as np
import pytest

import backend_patterns as BP
import bow_patterns as WP
import init_patterns as IP
import knn_patterns as KP
import sbow_patterns as OP
import sbp_patterns as P
import sbp_two_patterns as P2
import test_gpu_backend_adversarial as TB
import test_gpu_bow_adversarial as TW
import test_gpu_bow_slabs as TWS
import test_gpu_frustum_adversarial as TF
import test_gpu_fuse_batch as TFB
import test_gpu_init_adversarial as TI
import test_gpu_knn_adversarial as TK
import test_gpu_sbow_adversarial as TO
import test_gpu_sbp_adversarial as TS
import test_gpu_sbp_kf_batch as TKB
import test_gpu_sbp_two_adversarial as TS2
import test_gpu_tri_batch as TTB
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.matcher import DeviceMatchFrame, MatchFrame, ORBmatcher, search_by_projection_local_device
# module-scoped fixtures of the suites whose runners need them, under names of this module's own
from test_gpu_frustum_adversarial import expected as frustum_expected  # noqa: F401
from test_gpu_frustum_adversarial import om  # noqa: F401
from test_gpu_fuse_batch import strangers as fuse_strangers  # noqa: F401
from test_gpu_tri_batch import strangers as tri_strangers  # noqa: F401

pytestmark = pytest.mark.gpu

WORDS = [0, 1]
MIB = 1 << 20


def _first(cases, key):
    """The first case of every distinct key, in the module's order."""
    seen, out = set(), []
    for c in cases:
        k = key(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


# the kinds that pick a kernel form: (local, th 1 / 3 / 5), last frame, keyframe
SBP = _first(P.all_cases(), lambda c: (c.kind, c.par["th"] if c.kind == "local" else None))
SBP2 = _first(TS2.CASES, lambda c: c.kind)
KFF, KFKF = TO.KFF[0], TO.KFKF[0]
INIT = TI.CASES[0]
BACKEND = _first(TB.CASES, lambda c: c.entry)
KNN = KP.all_cases()[0]
BOW = TW.CASES[0]


def fill(word):
    out = (ctypes.c_int64 * 3)(-1, -1, -1)
    assert _lib.load().orbfe_debug_fill_matcher(word, out) == _lib.ORBFE_OK
    return list(out)


class Ctx:
    """What the runners need, and the oracle's answers, computed once per module."""

    def __init__(self, gpu, oracle, frustum, fuse_str, tri_str):
        self.gpu, self.om, self.lib = gpu, oracle, _lib.load()
        self.frustum, self.fuse_str, self.tri_str = frustum, fuse_str, tri_str
        self.cache, self.forms, self.vocs = {}, {}, {}

    def oracle(self, key, fn):
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]

    def ran(self, family, form):
        self.forms.setdefault(family, set()).add(form)

    def voc(self, voc):
        if id(voc) not in self.vocs:
            self.vocs[id(voc)] = (voc, voc.device())
        return self.vocs[id(voc)][1]

    def close(self):
        for _, gv in self.vocs.values():
            gv.close()


@pytest.fixture(scope="module")
def ctx(gpu, oracle_lib, frustum_expected, fuse_strangers, tri_strangers):
    c = Ctx(gpu, oracle_lib, frustum_expected, fuse_strangers, tri_strangers)
    yield c
    print("forms that ran, by family:", {k: sorted(v, key=str) for k, v in sorted(c.forms.items())})
    c.close()


# ---- the runners: each makes one call (or one suite's calls for a case), compares with the oracle and asserts the form
def run_sbp(ctx, case, padded, tag=""):
    want = ctx.oracle(("sbp", case.name + tag), lambda: P.run_oracle(ctx.om, case))
    c = case if padded is None else P.pad_queries(case) if padded == "queries" else P.pad_keys(case)
    form, _ = TS._form(case, padded)
    n, mvp = TS._run_gpu(c)
    got = ctx.lib.orbfe_matcher_last_form()
    assert got == form, (case.name, padded, got, form)
    assert n == want[0], (case.name, padded, n, want[0])
    np.testing.assert_array_equal(mvp[:case.F.N], want[1], err_msg=f"{case.name} {padded}")
    assert (mvp[case.F.N:] == -1).all(), (case.name, padded)
    ctx.ran("sbp " + case.kind, f"form {form} ({padded or 'planted'})")


class DeviceCase:
    """A local-map case's arrays in HBM, made once: a device-resident call then enqueues nothing but itself."""

    def __init__(self, gpu, case):
        import torch
        self.case, self.Fd = case, DeviceMatchFrame(case.F, gpu)
        self.mvp0 = torch.from_numpy(case.mvp0.copy()).to(gpu)
        self.obs = torch.from_numpy(case.obs.copy()).to(gpu)
        self.mps = torch.from_numpy(case.q.view(np.uint8).reshape(-1).copy()).to(gpu)
        self.mvp = self.mvp0.clone()

    def launch(self):
        """On the current torch stream; the slots stay on the device (read them with slots())."""
        self.mvp.copy_(self.mvp0)
        return search_by_projection_local_device(self.Fd, self.mvp, self.obs, self.mps, self.case.par["th"],
                                                 nnratio=self.case.par["nnratio"])

    def slots(self):
        return self.mvp.cpu().numpy()


def _padded(case, padded):
    return case if padded is None else P.pad_queries(case) if padded == "queries" else P.pad_keys(case)


def run_sbp_device(ctx, case, padded=None, tag=""):
    """Device-resident: as planted the one-workgroup form on the caller's arrays; padded to 2,049 the multi-launch
    forms, whose passes work in the thread's arena and whose last commit block the call does not wait for."""
    want = ctx.oracle(("sbp", case.name + tag), lambda: P.run_oracle(ctx.om, case))
    d = ctx.oracle(("sbp-dev", case.name + tag, padded), lambda: DeviceCase(ctx.gpu, _padded(case, padded)))
    form, _ = TS._form(case, padded)
    n = d.launch()
    got = ctx.lib.orbfe_matcher_last_form()
    assert got == form, (case.name, padded, got, form)
    assert n == want[0], (case.name, padded, n, want[0])
    s = d.slots()
    np.testing.assert_array_equal(s[:case.F.N], want[1], err_msg=f"{case.name} device-resident {padded}")
    assert (s[case.F.N:] == -1).all(), (case.name, padded)
    ctx.ran("sbp local", f"form {form} (device-resident, {padded or 'planted'})")


def run_sbp2(ctx, case, padded, tag=""):
    want = ctx.oracle(("sbp2", case.name + tag), lambda: P2.run_oracle(ctx.om, case))
    c = case if padded is None else P2.pad_queries(case) if padded == "queries" else P2.pad_keys(case)
    form = TS2._form(case, padded)
    n, mvp, got = TS2._run_gpu(ORBmatcher(), c)
    assert got == form, (case.name, padded, got, form)
    assert n == want[0], (case.name, padded, n, want[0])
    np.testing.assert_array_equal(mvp[:case.F.N], want[1], err_msg=f"{case.name} {padded}")
    assert (mvp[case.F.N:] == -1).all(), (case.name, padded)
    ctx.ran("sbp_two " + case.kind, f"form {form} ({padded or 'planted'})")


def run_kff(ctx, which, case=None, tag=""):
    case = KFF if case is None else case
    want = ctx.oracle(("sbow", case.name + tag), lambda: OP.run_oracle(ctx.om, case))
    c, form = {"planted": (case, TO.FORM_BLOCK), "frame": (OP.pad_frame(case), TO.FORM_NODES),
               "keyframe": (OP.pad_keyframe(case), TO.FORM_NODES)}[which]
    n, s = ORBmatcher(case.nnratio, case.check_ori).SearchByBoW(c.a.keys, c.a.desc, c.a.mp, c.a.fv, c.F, c.b.fv)
    assert ctx.lib.orbfe_matcher_last_bow_form() == form, (which, ctx.lib.orbfe_matcher_last_bow_form())
    assert n == want[0], (case.name, which, n, want[0])
    np.testing.assert_array_equal(s[:case.b.N], want[1], err_msg=f"{case.name} {which}")
    assert (s[case.b.N:] == -1).all()
    ctx.ran("sbow kf-f", f"bow form {form} ({which})")


def run_kff_batch(ctx, device, case=None, tag=""):
    """One SearchByBoWBatch call: [the keyframe, a discarded candidate, an empty keyframe, the padded keyframe]
    against the case's F on the host or in HBM (the call of test_gpu_sbow_adversarial.test_kf_f_batch)."""
    from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
    from orb_slam3_ros_amd.matcher import FeatureVector, KeyFrameFeatures
    case = KFF if case is None else case
    n_o, s_o = ctx.oracle(("sbow", case.name + tag), lambda: OP.run_oracle(ctx.om, case))
    big = OP.pad_keyframe(case)
    empty = MatchFrame(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), OP.BOUNDS, OP.SF)
    kfs = [KeyFrameFeatures(TO._kf_frame(case.a), case.a.fv), None, KeyFrameFeatures(empty, FeatureVector({})),
           KeyFrameFeatures(TO._kf_frame(big.a), big.a.fv)]
    try:
        F = case.F
        if device:
            F = DeviceMatchFrame(case.F, ctx.gpu)
            F.c.device = 1
        nm, rows = ORBmatcher(case.nnratio, case.check_ori).SearchByBoWBatch(
            kfs, [case.a.mp, None, np.zeros(0, np.int32), big.a.mp], F, case.b.fv)
        assert TO._batch_counts(ctx.lib) == (1, 2, 1)
        assert nm.tolist() == [n_o, 0, 0, n_o]
        np.testing.assert_array_equal(rows[0], s_o)
        np.testing.assert_array_equal(rows[3], s_o)
        assert (rows[1:3] == -1).all()
    finally:
        for k in kfs:
            if k is not None:
                k.close()
    ctx.ran("sbow kf-f", "SearchByBoWBatch rows (1, 2, 1), F " + ("in HBM" if device else "on the host"))


def run_kfkf(ctx, which, case=None, tag=""):
    case = KFKF if case is None else case
    n_o, s_o = ctx.oracle(("sbow", case.name + tag), lambda: OP.run_oracle(ctx.om, case))
    c = {"planted": case, "frame": OP.pad_frame(case), "keyframe": OP.pad_keyframe(case)}[which]
    a, b = c.a, c.b
    n, s = ORBmatcher(case.nnratio, case.check_ori).SearchByBoWKF(
        a.keys, a.desc, a.mp, a.fv, b.keys, b.desc, b.mp, b.fv, -1 if a.nleft is None else a.nleft,
        -1 if b.nleft is None else b.nleft)
    assert ctx.lib.orbfe_matcher_last_bow_form() == TO.FORM_KFKF
    assert n == n_o, (c.name, n, n_o)
    np.testing.assert_array_equal(s[:case.a.N], s_o, err_msg=c.name)
    assert (s[case.a.N:] == -1).all(), c.name
    ctx.ran("sbow kf-kf", f"bow form {TO.FORM_KFKF} ({which})")


def run_kfkf_batch(ctx, case=None):
    TO.test_kf_kf_batch(ctx.lib, ctx.om, KFKF if case is None else case)   # one SearchByBoWKFBatch call
    ctx.ran("sbow kf-kf", "SearchByBoWKFBatch (rows 0, 1, 2)")


def run_slabs(ctx, case=None, tag=""):
    """One SearchByBoWSlabs call: the keyframe as planted (LDS form) and padded (HBM form) against the frame and
    two decoys (the first call of test_gpu_bow_slabs.test_every_rule_both_forms)."""
    case = TWS.KFF1[0] if case is None else case
    n_o, s_o = ctx.oracle(("slabs", case.name + tag), lambda: OP.run_oracle(ctx.om, case))
    kf, F = TWS.of_side(case.a), TWS.of_side(case.b)
    big = TWS.pad_keyframe(kf, TWS.PAD)
    rng = np.random.default_rng(len(case.name))
    decoys = [TWS.Feats(F.keys, rng.integers(0, 256, (F.N, 32), dtype=np.uint8), F.fv) for _ in range(2)]
    exp, rows, forms = TWS.check(ctx.gpu, ctx.om, [decoys[0], F, decoys[1]], [(1, kf), (1, big), (0, kf), (2, big)],
                                 0, 1, case.nnratio, case.check_ori)
    assert forms == [0, 2, 0, 2], forms
    assert exp[0] == exp[1] == n_o
    np.testing.assert_array_equal(rows[0, :F.N], s_o)
    np.testing.assert_array_equal(rows[1, :F.N], s_o)
    ctx.ran("sbow kf-f", "SearchByBoWSlabs (LDS and HBM rows of one launch)")


def run_init(ctx, case=None, tag=""):
    case = INIT if case is None else case
    want = ctx.oracle(("init", case.name + tag), lambda: IP.run_definition(case)[:3])
    TI._assert_equal(TI._run(case), want, case.name)
    ctx.ran("init", "SearchForInitialization")


def run_knn(ctx, case=None, tag=""):
    c = KNN if case is None else case
    want = ctx.oracle(("knn", c.name + tag), lambda: ctx.om.stereo_knn_ratio(c.L, c.R, c.ratio))
    n, t, d = TK.stereo_knn_ratio(c.L, c.R, c.ratio)
    np.testing.assert_array_equal(t, want[1], err_msg=c.name)
    np.testing.assert_array_equal(d, want[2], err_msg=c.name)
    assert n == want[0] == int((t >= 0).sum()), c.name
    ctx.ran("knn", "k_knn2 (host call)")


def run_knn_slabs(ctx, nframes):
    (cap, ratio), frames = sorted(KP.launch_groups().items())[0]
    chunk = next(iter(KP.launches(frames, nframes)))
    TK._launch(ctx.lib, ctx.gpu, ctx.om, chunk, KP.ADDRESSINGS[0], twice=False)   # asserts orbfe_matcher_last_knn_form
    ctx.ran("knn", f"k_knn2_batch<{16 if nframes < 16 else 4}> ({len(chunk)} frames)")


BOW_FORMS = ("transform", "compute_bow(host)", "compute_bow(device)", "compute_bow(view)")


def run_bow(ctx, form, desc=None, tag=""):
    desc = BOW.desc if desc is None else desc
    want = ctx.oracle(("bow", BOW.name + tag), lambda: WP.run_definition(BOW, desc=desc)[:2])
    TW._same(TW._forms(ctx.gpu, ctx.voc(BOW.voc), BOW.levelsup)[form](desc), want, f"{BOW.name} {form}{tag}")
    ctx.ran("bow", form)


def run_bow_batch(ctx, desc=None, tag=""):
    """One transform_batch call over [the image, its first half, the image]."""
    desc = BOW.desc if desc is None else desc
    half = desc[:max(1, len(desc) // 2)]
    want = ctx.oracle(("bow", BOW.name + tag), lambda: WP.run_definition(BOW, desc=desc)[:2])
    want_half = ctx.oracle(("bow-half", BOW.name + tag), lambda: WP.run_definition(BOW, desc=half)[:2])
    cap = len(desc) + 3
    out = TW._batch(ctx.gpu, ctx.voc(BOW.voc), BOW.voc, [desc, half, desc], [len(desc), len(half), len(desc)], cap,
                    BOW.levelsup, None)
    for i, w in ((0, want), (1, want_half), (2, want)):
        TW._same(out.host(i), w, f"{BOW.name} batch image {i}{tag}")
    ctx.ran("bow", "transform_batch")


BACKEND_FORMS = ("planted", "pinhole", "points", "keys")


def backend_forms(c):
    return [f for f in BACKEND_FORMS if f != "pinhole" or c.entry in ("fuse", "fuse-sim3", "sbp", "sbp-kfs")]


def run_backend(ctx, case, form, tag=""):
    want = ctx.oracle(("backend", case.name + tag), lambda: BP.run_oracle(ctx.om, case))
    if form in ("planted", "pinhole"):
        TB._equal(TB._run_gpu(case, model=TB.PINHOLE if form == "pinhole" else None), want, f"{case.name} {form}")
    else:
        padded = BP.pad_points(case) if form == "points" else BP.pad_keys(case)
        want_p = ctx.oracle(("backend", padded.name + tag), lambda: BP.run_oracle(ctx.om, padded))
        got = TB._run_gpu(padded)
        TB._equal(got, want_p, padded.name)
        assert got[0] == want[0]
        for a, b in zip(got[1:], want[1:]):
            np.testing.assert_array_equal(a[:len(b)], b, err_msg=padded.name)
            assert (a[len(b):] == -1).all(), padded.name
    ctx.ran("backend " + case.entry, form)


def run_tri_batch(ctx):
    """One SearchForTriangulationBatch call: the case as the last job behind two unrelated neighbours."""
    from orb_slam3_ros_amd.matcher import FeatureVector
    c = TTB.TRI[0]
    want = ctx.oracle(("tri-batch", c.name), lambda: BP.run_oracle(ctx.om, c))
    k1 = TTB.Res(c.K1, FeatureVector(c.fv1), c.mp1)
    k2 = TTB.Job(TTB.Res(c.K2, FeatureVector(c.fv2), c.mp2, c.sigma2), c.F12, c.ep)
    try:
        exp_n, exp = TTB._check(ctx.om, k1, ctx.tri_str + [k2], c.only_stereo, c.coarse, c.check_ori)
        assert exp_n[2] == want[0]
        np.testing.assert_array_equal(exp[2], want[1])
    finally:
        k1.close()
        k2.res.close()
    ctx.ran("backend tri", "SearchForTriangulationBatch")


def run_frustum_fused(ctx, c=None, F=None, pts=None, tag=""):
    """search_local_points(track=True): nmatches, nToMatch and the slots against the oracle on the same inputs."""
    c = TF.SEARCHED[0] if c is None else c
    F = ctx.frustum[c.name]["F"] if F is None else F
    pts = c.flagged() if pts is None else pts

    def oracle():
        mvp, obs = np.full(F.N, -1, np.int32), np.zeros(F.N, np.int32)
        n, ntm = ctx.om.search_local_points(F, c.cam, pts, mvp, obs, c.th, False, 50.0, 0.8, c.rig)
        return n, ntm, mvp
    want = ctx.oracle(("frustum-fused", c.name + tag), oracle)
    mvp, obs = np.full(F.N, -1, np.int32), np.zeros(F.N, np.int32)
    n, ntm, _ = TF.search_local_points(F, c.cam, pts, mvp, obs, c.th, False, 50.0, 0.8, c.rig, track=True)
    assert (n, ntm) == want[:2], (c.name, n, ntm, want[:2])
    np.testing.assert_array_equal(mvp, want[2], err_msg=c.name + tag)
    ctx.ran("frustum", "fused host call with records")


def _one(family, form, fn):
    """A runner of another suite that makes exactly one matcher call."""
    def run(ctx):
        fn(ctx)
        ctx.ran(family, form)
    return run


def steps():
    """(id, uses device-resident inputs, runner): every selected case in every form its suite drives, one matcher
    call (one launch chain) per step, so that a fill in front of a step is a fill in front of that form."""
    out = []
    for c in SBP:
        for padded in (None, "queries", "keys"):
            out.append((f"sbp-{c.name}-{padded or 'planted'}", False, lambda x, c=c, p=padded: run_sbp(x, c, p)))
        if c.kind == "local":
            for padded in (None, "queries", "keys"):
                out.append((f"sbp-{c.name}-device-{padded or 'planted'}", True,
                            lambda x, c=c, p=padded: run_sbp_device(x, c, p)))
    for c in SBP2:
        for padded in (None, "queries", "keys"):
            out.append((f"sbp2-{c.name}-{padded or 'planted'}", False, lambda x, c=c, p=padded: run_sbp2(x, c, p)))
    for which in ("planted", "frame", "keyframe"):
        out.append((f"sbow-kff-{which}", False, lambda x, w=which: run_kff(x, w)))
        out.append((f"sbow-kfkf-{which}", False, lambda x, w=which: run_kfkf(x, w)))
    out += [
        ("sbow-kff-batch-host", False, lambda x: run_kff_batch(x, False)),
        ("sbow-kff-batch-device", True, lambda x: run_kff_batch(x, True)),
        ("sbow-kfkf-batch", False, run_kfkf_batch),
        ("sbow-slabs", True, run_slabs),
        ("init", False, run_init),
        ("knn-host", False, run_knn),
        ("knn-slabs-1", True, lambda x: run_knn_slabs(x, 1)),
        ("knn-slabs-16", True, lambda x: run_knn_slabs(x, 16)),
        ("bow-batch", True, run_bow_batch),
    ]
    for f in BOW_FORMS:
        out.append((f"bow-{f}", f != "transform", lambda x, f=f: run_bow(x, f)))
    for c in BACKEND:
        for f in backend_forms(c):
            out.append((f"backend-{c.entry}-{f}", False, lambda x, c=c, f=f: run_backend(x, c, f)))
    out += [
        ("fuse-batch", False, _one("backend fuse", "FuseBatch",
                                   lambda x: TFB.test_planted_rules(x.gpu, x.om, x.fuse_str, TFB.FUSE[0]))),
        ("tri-batch", False, run_tri_batch),
        ("kf-batch", False, _one("sbp kf", "SearchByProjectionKFBatch",
                                 lambda x: TKB.test_three_poses(x.gpu, x.om, *TKB.SWEEPS[0], True))),
        ("frustum", False, _one("frustum", "k_frustum", lambda x: TF.test_k_frustum(x.gpu, x.frustum, TF.FRUSTUM[0]))),
        ("frustum-fused", False, run_frustum_fused),
        ("frustum-device", True, _one("frustum", "fused device-resident call",
                                      lambda x: TF.test_fused_device_resident(x.gpu, x.frustum, TF.SEARCHED[0]))),
        ("local-batch", True, _one("frustum", "SearchLocalPointsBatch (k_local_batch)",
                                   lambda x: TF.test_k_local_batch(x.gpu, x.frustum, TF.GROUPS[0]))),
        ("last-proj", False, _one("frustum", "SearchByProjectionLastFramePose (k_last_proj)",
                                  lambda x: TF.test_k_last_proj(x.gpu, x.om, TF.LAST[0]))),
        ("track-batch", True, _one("frustum", "SearchByProjectionLastFrameBatch (trk_query)",
                                   lambda x: TF.test_trk_query(x.gpu, x.om, TF.track_groups()[0]))),
    ]
    return out


STEPS = steps()


# ---- poisoned arena, every form ------------------------------------------------------------------------------
@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("k", range(len(STEPS)), ids=[s[0] for s in STEPS])
def test_poisoned_arena(ctx, k, word):
    """The call once (it sizes the arena), the three blocks filled with `word`, the call again."""
    name, _, run = STEPS[k]
    run(ctx)
    nbytes = fill(word)
    print(f"{name} word {word}: orbfe_debug_fill_matcher filled {nbytes} bytes (arena, staging, slots)")
    assert nbytes[0] > 0 and all(b >= 0 and b % 4 == 0 for b in nbytes), nbytes
    run(ctx)
    fill(word)
    run(ctx)


def test_fill_reaches_all_three_blocks(ctx):
    """Non-vacuity: after a one-workgroup search (mapped staging, mapped slots) and a padded one (the arena) all
    three byte counts are positive and the arena is at least its 1 MiB floor."""
    run_sbp(ctx, SBP[0], None)
    run_sbp(ctx, SBP[0], "keys")
    nbytes = fill(1)
    assert all(b > 0 for b in nbytes) and nbytes[0] >= MIB, nbytes
    run_sbp(ctx, SBP[0], None)
    run_sbp(ctx, SBP[0], "keys")


# ---- same-shape predecessor ----------------------------------------------------------------------------------
# A sibling has the case's n and nq and other content: every descriptor complemented and the queries (or what
# stands for them: the points, the keyframe's map points, the image's features) reversed where the case's index
# structures allow it. Its answer is compared with the oracle's on the sibling itself.
def _clone(case, **kw):
    c = object.__new__(type(case))
    c.__dict__.update(case.__dict__)
    c.__dict__.update(kw)
    return c


def _not(a):
    return np.ascontiguousarray(~np.asarray(a, np.uint8))


def _frame_not(F):
    return MatchFrame(F.keys, _not(F.desc), F.bounds, F.scale_factors, F.uright, F.mbf, F.nleft,
                      getattr(F, "l2r", None), getattr(F, "r2l", None))


def _records_not(r, reverse):
    r = (r[::-1] if reverse else r).copy()
    if r.dtype.names and "desc" in r.dtype.names:
        r["desc"] = ~r["desc"]
    return r


def _sibling_sbp(case):
    kw = dict(q=_records_not(case.q, True), F=_frame_not(case.F))
    if getattr(case, "ruv", None) is not None:
        kw["ruv"] = np.ascontiguousarray(case.ruv[::-1])
    return _clone(case, **kw)


def _sibling_sbow(case):
    """Both sides' descriptors complemented, the keyframe's map points reversed (which features hold one)."""
    a = _clone(case.a, desc=_not(case.a.desc), mp=np.ascontiguousarray(case.a.mp[::-1]))
    b = _clone(case.b, desc=_not(case.b.desc))
    kw = dict(a=a, b=b)
    if getattr(case, "F", None) is not None:
        kw["F"] = _frame_not(case.F)
    return _clone(case, **kw)


def _sibling_backend(case):
    """Every frame's descriptors and every point record's descriptor complemented; the Fuse point list reversed
    (the other entries index their points from arrays of the case, which stay as they are)."""
    kw = {}
    for k, v in case.__dict__.items():
        if isinstance(v, MatchFrame):
            kw[k] = _frame_not(v)
        elif isinstance(v, np.ndarray) and v.dtype.names and "desc" in v.dtype.names:
            kw[k] = _records_not(v, k == "pts" and case.entry in ("fuse", "fuse-sim3"))
    assert kw, case.name
    return _clone(case, **kw)


@pytest.mark.parametrize("padded", [None, "queries", "keys"], ids=["planted", "queries", "keys"])
@pytest.mark.parametrize("k", range(len(SBP)), ids=[c.name for c in SBP])
def test_same_shape_predecessor_sbp(ctx, k, padded):
    case = SBP[k]
    sib = _sibling_sbp(case)
    assert sib.F.N == case.F.N and len(sib.q) == len(case.q)
    for _ in range(2):
        run_sbp(ctx, sib, padded, tag="~")
        run_sbp(ctx, case, padded)
    if case.kind == "local":
        for _ in range(2):
            run_sbp_device(ctx, sib, padded, tag="~")
            run_sbp_device(ctx, case, padded)


@pytest.mark.parametrize("padded", [None, "queries", "keys"], ids=["planted", "queries", "keys"])
@pytest.mark.parametrize("k", range(len(SBP2)), ids=[c.name for c in SBP2])
def test_same_shape_predecessor_sbp_two(ctx, k, padded):
    case = SBP2[k]
    sib = _sibling_sbp(case)
    assert sib.F.N == case.F.N and len(sib.q) == len(case.q)
    for _ in range(2):
        run_sbp2(ctx, sib, padded, tag="~")
        run_sbp2(ctx, case, padded)


@pytest.mark.parametrize("which", ["planted", "frame", "keyframe", "batch-host", "batch-device", "slabs"])
def test_same_shape_predecessor_sbow_kff(ctx, which):
    case = TWS.KFF1[0] if which == "slabs" else KFF
    sib = _sibling_sbow(case)
    assert (sib.a.N, sib.b.N) == (case.a.N, case.b.N)
    for c, tag in ((sib, "~"), (case, ""), (sib, "~"), (case, "")):
        if which == "slabs":
            run_slabs(ctx, c, tag)
        elif which.startswith("batch"):
            run_kff_batch(ctx, which == "batch-device", c, tag)
        else:
            run_kff(ctx, which, c, tag)


@pytest.mark.parametrize("which", ["planted", "frame", "keyframe"])
def test_same_shape_predecessor_sbow_kfkf(ctx, which):
    sib = _sibling_sbow(KFKF)
    for c, tag in ((sib, "~"), (KFKF, ""), (sib, "~"), (KFKF, "")):
        run_kfkf(ctx, which, c, tag)


@pytest.mark.parametrize("k", range(len(BACKEND)), ids=[c.entry for c in BACKEND])
def test_same_shape_predecessor_backend(ctx, k):
    case = BACKEND[k]
    sib = _sibling_backend(case)
    for form in backend_forms(case):
        for _ in range(2):
            run_backend(ctx, sib, form, tag="~")
            run_backend(ctx, case, form)


def test_same_shape_predecessor_frustum(ctx):
    """The fused SearchLocalPoints call after the same frame with complemented descriptors and the points reversed."""
    c = TF.SEARCHED[0]
    F, pts = ctx.frustum[c.name]["F"], c.flagged()
    F2, pts2 = _frame_not(F), _records_not(pts, True)
    for _ in range(2):
        run_frustum_fused(ctx, c, F2, pts2, tag="~")
        run_frustum_fused(ctx, c)


def test_same_shape_predecessor_k_frustum(ctx):
    """isInFrustum alone after the same pose with the points reversed (their descriptors complemented)."""
    c = TF.FRUSTUM[0]
    assert not c.nan
    cases = ((_records_not(c.flagged(), True), "~"), (c.flagged(), ""))
    for pts, tag in cases * 2:
        want = ctx.oracle(("k_frustum", c.name + tag), lambda: ctx.om.is_in_frustum(c.geom, c.cam, pts, c.rig))
        ntm, rec = TF.is_in_frustum(c.geom, c.cam, pts, c.rig)
        assert ntm == want[0], (c.name + tag, ntm, want[0])
        TF.P.assert_records_equal(rec, want[1])
    ctx.ran("frustum", "k_frustum")


def test_same_shape_predecessor_last_proj(ctx):
    """SearchByProjectionLastFramePose after the same frame with complemented descriptors and the last frame's
    points reversed and complemented; each compared with the oracle's row for its own inputs."""
    c = TF.LAST[0]
    sib = _clone(c, F=_frame_not(c.F), pts=_records_not(c.pts, True))
    assert sib.F.N == c.F.N and len(sib.pts) == len(c.pts)
    for x, tag in ((sib, "~"), (c, "")) * 2:
        n, row = ctx.oracle(("last-proj", c.name + tag), lambda: TF.last_expected(ctx.om, x))
        mvp, obs = np.full(x.F.N, -1, np.int32), np.zeros(x.F.N, np.int32)
        ng = ORBmatcher(0.9, False).SearchByProjectionLastFramePose(x.F, mvp, obs, x.pts, x.Tcw, x.model, x.th, x.fw,
                                                                    x.bw, x.Trl)
        assert ng == n, (c.name + tag, ng, n)
        np.testing.assert_array_equal(mvp, row, err_msg=c.name + tag)
    ctx.ran("frustum", "SearchByProjectionLastFramePose (k_last_proj)")


@pytest.mark.parametrize("form", BOW_FORMS + ("batch",))
def test_same_shape_predecessor_bow(ctx, form):
    """ComputeBoW after an image of the same size: the features reversed, every descriptor complemented."""
    sib = _not(BOW.desc[::-1])
    for d, tag in ((sib, "~"), (None, ""), (sib, "~"), (None, "")):
        if form == "batch":
            run_bow_batch(ctx, d, tag)
        else:
            run_bow(ctx, form, d, tag)


def test_same_shape_predecessor_knn(ctx):
    c = KNN
    sib = _clone(c, L=_not(c.L[::-1]), R=_not(c.R))
    for _ in range(2):
        run_knn(ctx, sib, tag="~")
        run_knn(ctx, c)


def test_same_shape_predecessor_init(ctx):
    """SearchForInitialization after a sibling with F1's keys reversed (with their prev-matched points) and every
    descriptor complemented."""
    c = INIT
    F1, F2 = c.F1, c.F2
    r = slice(None, None, -1)
    sib = _clone(c, F1=MatchFrame(F1.keys[r].copy(), _not(F1.desc[r]), F1.bounds, F1.scale_factors),
                 F2=MatchFrame(F2.keys, _not(F2.desc), F2.bounds, F2.scale_factors), prev=c.prev[r].copy())
    for _ in range(2):
        run_init(ctx, sib, tag="~")
        run_init(ctx, c)


# ---- cross-family interleaving -------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True], ids=["shuffled", "reversed"])
def test_cross_family_interleaving(ctx, reverse):
    """One pass over every selected case of every family in a seeded shuffled order, host and device-resident
    forms mixed, each compared; then the same order backwards."""
    order = np.random.default_rng(20240).permutation(len(STEPS)).tolist()
    if reverse:
        order = order[::-1]
    kinds = [STEPS[i][1] for i in order]
    assert any(a != b for a, b in zip(kinds, kinds[1:]))   # host and device forms do alternate somewhere
    for i in order:
        STEPS[i][2](ctx)


# ---- pass_hint independence ----------------------------------------------------------------------------------
def _passes(lib):
    w = (ctypes.c_longlong * 3)()
    assert lib.orbfe_matcher_last_stats(w) == _lib.ORBFE_OK
    return int(w[2])


def test_pass_hint_independence(ctx):
    """The band form (th >= 4) and the multi form (th < 4) batch their launches by the pass count of the thread's
    previous search of the same mode (a batch of hint + 1, at most 8): a ladder that needs more passes than any
    batch in front of a one-pass case, and the other way round, in both forms. The pass counts are asserted from
    the counting mode, so a change in the patterns cannot empty the test."""
    ctx.lib.orbfe_matcher_set_stats(1)
    try:
        for th, form in ((15, TS.FORM_BAND), (3, TS.FORM_MULTI)):
            many = P.ladder("local", th, 1)
            one = next(c for c in P.all_cases() if c.kind == "local" and c.par["th"] == (5 if th == 15 else 3))
            for order in ((many, one), (one, many), (many, many, one, one)):
                for c in order:
                    run_sbp(ctx, c, "queries")
                    assert ctx.lib.orbfe_matcher_last_form() == form
                    n = _passes(ctx.lib)
                    print(f"th {th} form {form} {c.name}: {n} passes")
                    # the ladder needs a pass per rung (13), more than the largest batch of 8; the other case
                    # settles in its first pass, which a fixed-point loop may confirm with one more
                    assert (n > 8) if c is many else (1 <= n <= 2), (c.name, th, n)
    finally:
        ctx.lib.orbfe_matcher_set_stats(0)


# ---- tail ordering -------------------------------------------------------------------------------------------
def test_tail_ordering(ctx):
    """A device-resident multi-launch local-map search (queries or keys padded to 2,049: its commit blocks work in
    the arena and the call returns before the last one retires) on torch stream A, at once a host-form search
    that reuses the arena, at once a device-resident search on stream B: 50 rounds, the cases and paddings
    alternating, every result compared. Nothing is synchronised between the three calls."""
    import torch
    local = [c for c in SBP if c.kind == "local"]
    assert len(local) >= 2
    pads = ("queries", "keys")
    dev = [{(i, p): DeviceCase(ctx.gpu, _padded(c, p)) for i, c in enumerate(local) for p in pads} for _ in range(2)]
    want = [P.run_oracle(ctx.om, c) for c in local]
    A, B = torch.cuda.Stream(ctx.gpu), torch.cuda.Stream(ctx.gpu)
    torch.cuda.synchronize()
    seen = set()
    for r in range(50):
        ia, ih, ib = r % len(local), (r + 1) % len(local), (r + 2) % len(local)
        pa, pb = pads[r % 2], pads[(r // 2) % 2]
        with torch.cuda.stream(A):
            na = dev[0][ia, pa].launch()
        fa = ctx.lib.orbfe_matcher_last_form()
        host = local[ih] if r % 3 == 0 else _padded(local[ih], pads[r % 2])
        nh, mvp_h = TS._run_gpu(host)
        with torch.cuda.stream(B):
            nb = dev[1][ib, pb].launch()
        fb = ctx.lib.orbfe_matcher_last_form()
        assert fa == TS._form(local[ia], pa)[0] and fb == TS._form(local[ib], pb)[0], (r, fa, fb)
        assert fa != TS.FORM_BLOCK and fb != TS.FORM_BLOCK
        seen |= {fa, fb}
        assert (na, nh, nb) == (want[ia][0], want[ih][0], want[ib][0]), r
        np.testing.assert_array_equal(mvp_h[:local[ih].F.N], want[ih][1], err_msg=f"round {r} host")
        with torch.cuda.stream(A):
            sa = dev[0][ia, pa].slots()
        with torch.cuda.stream(B):
            sb = dev[1][ib, pb].slots()
        for s, i, what in ((sa, ia, "A"), (sb, ib, "B")):
            np.testing.assert_array_equal(s[:local[i].F.N], want[i][1], err_msg=f"round {r} stream {what}")
            assert (s[local[i].F.N:] == -1).all()
    assert {TS.FORM_MULTI, TS.FORM_BAND, TS.FORM_LOCAL} <= seen, seen
