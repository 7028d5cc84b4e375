"""GPU parity of the batched SearchByBoW over device-resident keyframes (orbfe_keyframe_create +
orbfe_search_by_bow_batch: the candidates loop of Tracking::Relocalization, Tracking.cc:3680-3701,
in one launch, one workgroup per candidate). Every row is checked against the CPU oracle's
OracleMatcher.search_by_bow called once per candidate on the same arrays: nmatches[c] equal and
out[c] array-equal. The GPU is never compared with itself.

sm.synth_bow re-draws both word assignments on every call, so the cases here draw F's words once and
give every candidate feature that copies an F feature the word of its source.
"""
import numpy as np
import pytest

from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
from orb_slam3_ros_amd.matcher import FeatureVector, KeyFrameFeatures, MatchFrame, ORBmatcher

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def om(oracle_lib):
    return oracle_lib


def _fv(words):
    d = {}
    for i, wd in enumerate(np.asarray(words).tolist()):
        d.setdefault(int(wd) * 7 + 3, []).append(i)   # sparse ascending node ids, as sm.synth_bow
    return FeatureVector(d)


def _mono(F):
    return MatchFrame(F.keys, F.desc, F.bounds, F.scale_factors)


def _candidate(rng, F, wf, n_words, n=None):
    """Another view of F's scene (sm.perturbed_frame), resized to n features (cut, or padded with
    unrelated ones). Returns (frame, words): a copied feature has its source's word."""
    KF, src = sm.perturbed_frame(rng, _mono(F), rot=20.0, flip_p=0.05, drop=0.15)
    keys, desc = KF.keys, KF.desc
    if n is not None and n < KF.N:
        keys, desc, src = keys[:n].copy(), desc[:n].copy(), src[:n]
    elif n is not None and n > KF.N:
        X = sm.synth_frame(rng, n - KF.N, stereo=False)
        keys, desc = np.concatenate([keys, X.keys]), np.concatenate([desc, X.desc])
        src = np.concatenate([src, np.full(X.N, -1)])
    wk = rng.integers(0, n_words, len(keys))
    m = src >= 0
    wk[m] = wf[src[m]]
    return MatchFrame(keys, desc, F.bounds, F.scale_factors), wk


def _unrelated(rng, n, n_words):
    return sm.synth_frame(rng, n, stereo=False), rng.integers(0, n_words, n)


def _mp(rng, n, hole=0.25):
    return np.where(rng.random(n) < hole, -1, np.arange(n) + 100).astype(np.int32)


class _Cand:
    """One candidate: the host arrays the oracle reads, and the resident handle made from them."""

    def __init__(self, KF, fv, mp, handle_from=None):
        self.KF, self.fv, self.mp = KF, fv, mp
        self.h = KeyFrameFeatures(KF if handle_from is None else handle_from, fv)


def _check(om, cands, F, ff, check_ori, Fcall=None, nnratio=0.75):
    """One batch call over cands (None = a discarded candidate) against the oracle per candidate.
    Returns the oracle's (nmatches, rows)."""
    kfs = [None if c is None else c.h for c in cands]
    mps = [None if c is None else c.mp for c in cands]
    nm, out = ORBmatcher(nnratio, check_ori).SearchByBoWBatch(kfs, mps, F if Fcall is None else Fcall, ff)
    assert nm.shape == (len(cands),) and out.shape == (len(cands), F.N)
    exp_n, exp = [], []
    for c in cands:
        if c is None:
            exp_n.append(0)
            exp.append(np.full(F.N, -1, np.int32))
            continue
        no, oo = om.OracleMatcher(nnratio, check_ori).search_by_bow(c.KF.keys, c.KF.desc, c.mp, c.fv, F, ff)
        exp_n.append(no)
        exp.append(oo)
    np.testing.assert_array_equal(nm, np.asarray(exp_n, np.int32))
    np.testing.assert_array_equal(out, np.stack(exp) if exp else out)
    return np.asarray(exp_n), (np.stack(exp) if exp else out)


@pytest.mark.parametrize("words", [50, 400])
def test_parity_plain(gpu, om, words):
    """Six candidates of 1000 features against a 1000-feature frame: three views of F's scene, three
    unrelated frames over the same word range; both check_ori values."""
    rng = np.random.default_rng(1100 + words)
    F = sm.synth_frame(rng, 1000, stereo=False)
    wf = rng.integers(0, words, F.N)
    ff = _fv(wf)
    cands = []
    for c in range(6):
        KF, wk = _candidate(rng, F, wf, words) if c < 3 else _unrelated(rng, 1000, words)
        cands.append(_Cand(KF, _fv(wk), _mp(rng, KF.N)))
    for check_ori in (True, False):
        no, _ = _check(om, cands, F, ff, check_ori)
        # the relocalisation threshold (Tracking.cc:3693) falls on both sides inside the batch
        assert (no >= 15).any() and (no < 15).any()
    for c in cands:
        c.h.close()


def test_mixed_shapes(gpu, om):
    """F.N = 777 (no multiple of 4 or 1024) against, in one batch: one 300 x 777 node (the large-node
    path), 1200 features over 5000 words (one-feature nodes, many without a partner), a discarded
    candidate, an empty keyframe, a keyframe without map points, one sharing no node with F, and a
    64-feature one."""
    rng = np.random.default_rng(777)
    F = sm.synth_frame(rng, 777, stereo=False)
    ff1 = _fv(np.zeros(F.N, np.int64))
    wf = rng.integers(0, 5000, F.N)
    ff = _fv(wf)
    one, _ = _candidate(rng, F, wf, 1, n=300)
    many, wmany = _candidate(rng, F, wf, 5000, n=1200)
    nomp, wnomp = _candidate(rng, F, wf, 5000, n=500)
    absent, wabs = _candidate(rng, F, wf, 5000, n=400)
    small, wsmall = _candidate(rng, F, wf, 5000, n=64)
    empty = MatchFrame(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), F.bounds, F.scale_factors)

    def batch(one_words):
        return [_Cand(one, _fv(one_words), _mp(rng, 300)),
                _Cand(many, _fv(wmany), _mp(rng, 1200)),
                None,
                _Cand(empty, FeatureVector({}), np.zeros(0, np.int32)),
                _Cand(nomp, _fv(wnomp), np.full(500, -1, np.int32)),
                _Cand(absent, _fv(wabs + 100000), _mp(rng, 400)),   # node ids above all of F's
                _Cand(small, _fv(wsmall), _mp(rng, 64))]
    for check_ori in (True, False):
        # F over 5000 words (candidate 0's single node is one of F's small nodes, or absent) ...
        cs = batch(np.full(300, wf[0]))
        no, _ = _check(om, cs, F, ff, check_ori)
        assert cs[3].h.N == 0 and no[2] == 0 and no[3] == 0 and no[4] == 0 and no[5] == 0 and no[1] > 0
        # ... and F as ONE node of 777 features against the 300-feature node
        cs1 = batch(np.zeros(300, np.int64))
        no1, _ = _check(om, cs1, F, ff1, check_ori)
        assert no1[0] > 0
        for c in cs + cs1:
            if c is not None:
                c.h.close()


@pytest.mark.parametrize("fn,big", [
    (2600, 2600),   # the middle candidate does not fit 150 KB of LDS: the multi-launch path inside a batch
    (3600, 2600),   # F just under the frame-side bound (40 B of LDS per F feature: fn <= ~3800) ...
    (4000, 2600),   # ... and above it (and under fn <= 4096): no candidate fits, all rows multi-launch
])
def test_fallback_inside_a_batch(gpu, om, fn, big):
    """Candidates of 200, 2600 and 64 features and a discarded one. The one-workgroup form needs
    40 B of LDS per F feature before any keyframe byte, so its fn <= 4096 bound is never the binding
    one: the bound as implemented is the LDS budget, with F.N = 3600 below it (only the 64-feature
    candidate still fits beside F) and F.N = 4000 above it."""
    rng = np.random.default_rng(fn)
    F = sm.synth_frame(rng, fn, stereo=False)
    words = 400
    wf = rng.integers(0, words, F.N)
    ff = _fv(wf)
    cands = []
    for n in (200, big, 64):
        KF, wk = _candidate(rng, F, wf, words, n=n)
        cands.append(_Cand(KF, _fv(wk), _mp(rng, n)))
    cands.insert(2, None)
    for check_ori in (True, False):
        no, _ = _check(om, cands, F, ff, check_ori)
        assert no[1] > 100 and no[0] > 0
    for c in cands:
        if c is not None:
            c.h.close()


def test_ties(gpu, om):
    """Identical descriptors inside a node: 3-5 F features equal one KF feature (the first by position
    wins, and the ratio test sees distance 0 twice), and two KF features of a node are equal (the
    second meets the "already matched" skip)."""
    rng = np.random.default_rng(4141)
    words = 60
    F = sm.synth_frame(rng, 600, stereo=False)
    wf = rng.integers(0, words, F.N)
    cands = []
    for c in range(3):
        KF, wk = _candidate(rng, F, wf, words)
        for w in rng.choice(words, 12, replace=False):
            fi, ki = np.nonzero(wf == w)[0], np.nonzero(wk == w)[0]
            if len(fi) < 5 or len(ki) < 2:
                continue
            k0 = ki[rng.integers(0, len(ki))]
            dup = rng.choice(fi, int(rng.integers(3, 6)), replace=False)
            F.desc[dup] = KF.desc[k0]
            if w % 2:   # near copies around one exact copy: equal second-best distances as well
                F.desc[dup[1:], 0] ^= 1
            k1 = ki[ki != k0][0]
            KF.desc[k1] = KF.desc[k0]
        cands.append((KF, wk))
    ff = _fv(wf)
    # F's descriptors changed after the candidates were drawn: handles are made now
    cs = [_Cand(KF, _fv(wk), _mp(rng, KF.N, hole=0.1)) for KF, wk in cands]
    for check_ori in (True, False):
        for ratio in (0.75, 0.95):
            no, _ = _check(om, cs, F, ff, check_ori, nnratio=ratio)
            assert (no > 0).all()
    for c in cs:
        c.h.close()


def test_two_camera_frame(gpu, om):
    """F.Nleft != -1: separate left / right best and second best, the right ratio test disabled."""
    rng = np.random.default_rng(52)
    F = sm.synth_frame_two(rng, 900, 900)
    for words in (50, 400):
        wf = rng.integers(0, words, F.N)
        lk = np.nonzero(F.l2r >= 0)[0]
        wf[900 + F.l2r[lk]] = wf[lk]   # a stereo pair sees one point: one word, so a KF feature meets both sides
        ff = _fv(wf)
        cs = []
        for n in (1000, 900, 1800):   # the last one does not fit a workgroup: the multi-launch path
            KF, wk = _candidate(rng, F, wf, words, n=n)
            cs.append(_Cand(KF, _fv(wk), _mp(rng, KF.N)))
        for check_ori in (True, False):
            no, rows = _check(om, cs, F, ff, check_ori)
            assert (no > 0).all() and (rows[:, 900:] >= 0).any(axis=1).all()   # right-camera matches
        for c in cs:
            c.h.close()


def test_reuse_and_staleness(gpu, om):
    """The same four handles over a sequence of calls: another frame (other N, other words), a
    shorter batch, map points that turned bad, a destroyed handle."""
    rng = np.random.default_rng(66)
    words = 300
    A = sm.synth_frame(rng, 1000, stereo=False)
    wa = rng.integers(0, words, A.N)
    cs, wks = [], []
    for c in range(4):
        KF, wk = _candidate(rng, A, wa, words, n=(1000, 700, 1000, 1300)[c])
        cs.append(_Cand(KF, _fv(wk), _mp(rng, KF.N)))
        wks.append(wk)
    B, srcb = sm.perturbed_frame(rng, cs[0].KF, rot=-15.0, flip_p=0.04, drop=0.3)
    B = MatchFrame(B.keys[:640].copy(), B.desc[:640].copy(), B.bounds, B.scale_factors)
    wb = rng.integers(0, words, B.N)   # other words: B sees keyframe 0's scene, not A's
    mb = srcb[:640] >= 0
    wb[mb] = wks[0][srcb[:640][mb]]
    fa, fb = _fv(wa), _fv(wb)
    na, _ = _check(om, cs, A, fa, True)
    assert (na > 0).all()
    nb0, _ = _check(om, cs, B, fb, True)
    assert (nb0 > 0).all()
    _check(om, [cs[2], cs[0]], A, fa, True)
    _check(om, [cs[1]], B, fb, False)
    for c in cs:
        c.mp = c.mp.copy()
        c.mp[rng.random(len(c.mp)) < 0.3] = -1
    nb, _ = _check(om, cs, A, fa, True)
    assert (nb < na).any()
    cs[1].h.close()
    assert cs[1].h.handle is None
    _check(om, [cs[0], None, cs[2], cs[3]], A, fa, True)
    with pytest.raises(ValueError):
        ORBmatcher(0.75).SearchByBoWBatch([cs[1].h], [cs[1].mp], A, fa)
    for c in cs:
        c.h.close()


def test_device_resident_inputs(gpu, om):
    """A keyframe handle made from the device view of an extracted frame (device-to-device copy) and
    one from the host copy of the same arrays; the frame passed as device view and as host view."""
    from orb_slam3_ros_amd import _lib
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_stereo
    from orb_slam3_ros_amd.matcher import current_frame_view
    from orb_slam3_ros_amd.synth import synth_stereo
    bf, fx = 0.110078 * 458.654, 458.654
    el, er = ORBextractor(1000, 1.2, 8, 20, 7), ORBextractor(1000, 1.2, 8, 20, 7)
    left, right = synth_stereo(5, 752, 480)
    (ml, kl, dl), _, ur, _, _ = frame_stereo(el, er, left, right, bf, fx)
    fid = _lib.load().orbfe_extractor_frame_id(el.handle)
    F = MatchFrame(kl, dl, (0.0, 752.0, 0.0, 480.0), np.asarray(el.GetScaleFactors(), np.float32), ur, bf)
    V = current_frame_view(F, el, fid)
    assert V is not None and V.N == F.N and F.N > 300
    rng = np.random.default_rng(8)
    words = 200
    wf = rng.integers(0, words, F.N)
    ff = _fv(wf)
    # the extracted frame itself as a keyframe (every feature meets its own copy), from HBM and from the host
    mp = _mp(rng, F.N)
    dev = _Cand(F, ff, mp, handle_from=V)
    host = _Cand(F, ff, mp)
    other_kf, wk = _candidate(rng, F, wf, words)
    other = _Cand(other_kf, _fv(wk), _mp(rng, other_kf.N))
    assert dev.h.N == F.N == host.h.N
    for check_ori in (True, False):
        n1, _ = _check(om, [dev, host, other], F, ff, check_ori, Fcall=V)
        n2, _ = _check(om, [dev, host, other], F, ff, check_ori)
        assert n1[0] == n1[1] > 100 and (n1 == n2).all()
    for c in (dev, host, other):
        c.h.close()


def test_handle_validation(gpu):
    """create refuses a FeatureVector orbfe_search_by_bow would refuse; orbfe_keyframe_n reports N."""
    from orb_slam3_ros_amd._lib import OrbfeError
    rng = np.random.default_rng(9)
    KF = sm.synth_frame(rng, 50, stereo=False)
    good = FeatureVector({3: [0, 1, 2], 10: [3, 49]})
    h = KeyFrameFeatures(KF, good)
    assert h.N == 50
    h.close()
    h.close()   # idempotent
    with pytest.raises(OrbfeError):
        KeyFrameFeatures(KF, FeatureVector({3: [0, 50]}))   # an index >= n
    desc = FeatureVector({3: [0, 1], 10: [2]})
    desc.node_ids[:] = [10, 3]   # descending node ids
    with pytest.raises(OrbfeError):
        KeyFrameFeatures(KF, desc)
    eq = FeatureVector({3: [0, 1], 10: [2]})
    eq.node_ids[:] = [3, 3]   # not strictly ascending
    with pytest.raises(OrbfeError):
        KeyFrameFeatures(KF, eq)
    off = FeatureVector({3: [0, 1], 10: [2]})
    off.offsets[0] = 1   # offsets[0] != 0
    with pytest.raises(OrbfeError):
        KeyFrameFeatures(KF, off)
    dec = FeatureVector({3: [0, 1], 10: [2], 11: [4]})
    dec.offsets[2] = 1   # decreasing offsets
    with pytest.raises(OrbfeError):
        KeyFrameFeatures(KF, dec)
