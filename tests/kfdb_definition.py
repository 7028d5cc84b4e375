"""TEST INFRASTRUCTURE (CPU only): a literal restatement of KeyFrameDatabase::add / erase
(KeyFrameDatabase.cc:39-66), DetectRelocalizationCandidates (:733-845) and L1Scoring::score
(ScoringObject.cpp:23-68). The inverted file is a list of lists, the per-keyframe query state
(mnRelocQuery, mnRelocWords, mRelocScore) persists between queries, Python float is the reference's
double and np.float32 every float variable of the reference. Also the fixtures the CPU and GPU
tests share."""
import bisect

import numpy as np

F32 = np.float32


class KF:
    """The fields of a KeyFrame the database touches."""

    def __init__(self, kf_id, bow, neighbours=(), map_id=0):
        self.mnId = int(kf_id)
        ids, w = bow
        self.words = [int(x) for x in ids]       # mBowVec: a std::map, ascending word ids
        self.weights = [float(x) for x in w]
        assert all(a < b for a, b in zip(self.words, self.words[1:]))
        self.neighbours = list(neighbours)       # GetBestCovisibilityKeyFrames(10): KF objects or ids
        self.map_id = map_id                     # GetMap()
        self.mnRelocQuery = -1
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)


def l1_score(v1_ids, v1_w, v2_ids, v2_w):
    """L1Scoring::score: the merge walk with lower_bound jumps, one double chain."""
    i1, i2 = 0, 0
    n1, n2 = len(v1_ids), len(v2_ids)
    score = 0.0
    while i1 != n1 and i2 != n2:
        vi, wi = v1_w[i1], v2_w[i2]
        if v1_ids[i1] == v2_ids[i2]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i1 += 1
            i2 += 1
        elif v1_ids[i1] < v2_ids[i2]:
            i1 = bisect.bisect_left(v1_ids, v2_ids[i2])
        else:
            i2 = bisect.bisect_left(v2_ids, v1_ids[i1])
    score = -score / 2.0
    return score


def shared_terms(v1_ids, v1_w, v2_ids, v2_w):
    """The addends of l1_score's chain, in the order it adds them."""
    w2 = dict(zip(v2_ids, v2_w))
    return [abs(a - w2[i]) - abs(a) - abs(w2[i]) for i, a in zip(v1_ids, v1_w) if i in w2]


class KeyFrameDatabaseDef:
    def __init__(self, n_words):
        self.mvInvertedFile = [[] for _ in range(n_words)]
        self.kfs = {}          # id -> KF (the caller's keyframe table)
        self.next_query = 0    # F->mnId

    def add(self, kf):
        assert kf.mnId not in self.kfs
        self.kfs[kf.mnId] = kf
        for w in kf.words:
            self.mvInvertedFile[w].append(kf)

    def erase(self, kf_id):
        kf = self.kfs.pop(kf_id)
        for w in kf.words:
            lst = self.mvInvertedFile[w]
            for i, other in enumerate(lst):
                if other is kf:
                    del lst[i]
                    break

    def _resolve(self, x):
        return x if isinstance(x, KF) else self.kfs.get(x)

    def _stage12(self, bow):
        f_ids = [int(x) for x in bow[0]]
        f_w = [float(x) for x in bow[1]]
        fid = self.next_query
        self.next_query += 1
        lKFsSharingWords = []
        for w in f_ids:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != fid:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = fid
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > maxCommonWords:
                maxCommonWords = pKFi.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(l1_score(f_ids, f_w, pKFi.words, pKFi.weights))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        return fid, lKFsSharingWords, maxCommonWords, lScoreAndMatch

    def shared_words(self, bow):
        """-> (kf ids, words, scores, scored, maxCommonWords) in the list order."""
        _, lst, mx, sm = self._stage12(bow)
        passed = {id(k): s for s, k in sm}
        ids = np.array([k.mnId for k in lst], np.int32)
        words = np.array([k.mnRelocWords for k in lst], np.int32)
        scored = np.array([id(k) in passed for k in lst], bool)
        scores = np.array([passed.get(id(k), F32(0)) for k in lst], np.float32)
        return ids, words, scores, scored, mx

    def DetectRelocalizationCandidates(self, bow, map_id=0):
        fid, lst, _, lScoreAndMatch = self._stage12(bow)
        if not lst or not lScoreAndMatch:
            return np.zeros(0, np.int32)
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for nb in pKFi.neighbours[:10]:
                pKF2 = self._resolve(nb)
                if pKF2 is None or pKF2.mnRelocQuery != fid:
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        added = set()
        out = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi.map_id != map_id:
                    continue
                if id(pKFi) not in added:
                    out.append(pKFi.mnId)
                    added.add(id(pKFi))
        return np.array(out, np.int32)


class KeyFrameDatabaseNative:
    """tests/native/kfdb_cpu.cpp (std::list / std::map, built by orb_slam3_ros_amd.build.build_kfdb_cpu)
    behind the interface of KeyFrameDatabaseDef."""

    def __init__(self, n_words):
        import ctypes
        from orb_slam3_ros_amd import build
        self.ct = ctypes
        self.lib = ctypes.CDLL(build.build_kfdb_cpu())
        vp, ci = ctypes.c_void_p, ctypes.c_int
        self.lib.kfdbcpu_create.restype = vp
        self.lib.kfdbcpu_create.argtypes = [ci]
        self.lib.kfdbcpu_destroy.restype = None
        self.lib.kfdbcpu_destroy.argtypes = [vp]
        self.lib.kfdbcpu_add.argtypes = [vp, ci, vp, vp, ci, vp, ci, ci]
        self.lib.kfdbcpu_erase.argtypes = [vp, ci]
        self.lib.kfdbcpu_shared_words.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp]
        self.lib.kfdbcpu_detect.argtypes = [vp, vp, vp, ci, ci, vp]
        self.lib.kfdbcpu_detect_reps.argtypes = [vp, vp, vp, ci, ci, ci]
        self.h = self.lib.kfdbcpu_create(int(n_words))
        self.n = 0

    @staticmethod
    def _bow(bow):
        return np.ascontiguousarray(bow[0], np.uint32), np.ascontiguousarray(bow[1], np.float64)

    def add(self, kf):
        ids = np.array(kf.words, np.uint32)
        w = np.array(kf.weights, np.float64)
        nb = np.array([x.mnId if isinstance(x, KF) else int(x) for x in kf.neighbours], np.int32)
        assert self.lib.kfdbcpu_add(self.h, kf.mnId, ids.ctypes.data, w.ctypes.data, len(ids), nb.ctypes.data, len(nb),
                                    int(kf.map_id)) == 0
        self.n += 1

    def erase(self, kf_id):
        assert self.lib.kfdbcpu_erase(self.h, int(kf_id)) == 0
        self.n -= 1

    def shared_words(self, bow):
        ids, w = self._bow(bow)
        cap = max(self.n, 1)
        kf, words = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        sc, fl = np.zeros(cap, np.float32), np.zeros(cap, np.uint8)
        mx = self.ct.c_int(0)
        n = self.lib.kfdbcpu_shared_words(self.h, ids.ctypes.data, w.ctypes.data, len(ids), kf.ctypes.data,
                                          words.ctypes.data, sc.ctypes.data, fl.ctypes.data, self.ct.addressof(mx))
        return kf[:n].copy(), words[:n].copy(), sc[:n].copy(), fl[:n].astype(bool), mx.value

    def DetectRelocalizationCandidates(self, bow, map_id=0):
        ids, w = self._bow(bow)
        out = np.zeros(max(self.n, 1), np.int32)
        n = self.lib.kfdbcpu_detect(self.h, ids.ctypes.data, w.ctypes.data, len(ids), int(map_id), out.ctypes.data)
        return out[:n].copy()

    def detect_reps(self, bow, reps, map_id=0):
        """reps queries inside one native call (no Python in the timed loop); -> candidates of the last."""
        ids, w = self._bow(bow)
        return self.lib.kfdbcpu_detect_reps(self.h, ids.ctypes.data, w.ctypes.data, len(ids), int(map_id), int(reps))

    def close(self):
        if self.h:
            self.lib.kfdbcpu_destroy(self.h)
            self.h = None


# ---- fixtures shared by tests/test_kfdb_definition.py, tests/test_kfdb_native.py, tests/test_gpu_kfdb.py ----

def random_bow(rng, n_words, n, l1=True):
    ids = np.sort(rng.choice(n_words, size=n, replace=False)).astype(np.uint32)
    w = rng.uniform(0.05, 1.0, n)
    if l1:
        w = w / np.abs(w).sum()
    return ids, w


def ordered_sum_fixture():
    """Weights spread over six decades, not normalised, some negative and some zero: the score's
    double chain depends on its order. -> (n_words, query bow, [keyframe bows]).

    The last keyframe makes the order visible in the float score as well. It shares words 0..101 with
    the query at equal weights 1, 2^-24 and 100 x 2^-54, so its terms are -2, -2^-23 and 100 x -2^-53.
    Left to right, -(2 + 2^-23) absorbs every -2^-53 (half an ulp there is 2^-52): the score is
    1 + 2^-24 exactly, a tie that rounds to float 1.0. Any order that adds two of the small terms to
    each other first (a reversed chain, a tree, per-chunk partial sums) keeps them, and the score
    rounds up to 1 + 2^-23."""
    rng = np.random.default_rng(61)
    n_words = 256
    lo = 102   # words 0..101 belong to the last keyframe

    def vec(n):
        ids = np.sort(lo + rng.choice(n_words - lo, size=n, replace=False)).astype(np.uint32)
        w = 10.0 ** rng.uniform(-3.0, 3.0, n) * rng.choice([1.0, 1.0, -1.0], n)
        w[rng.random(n) < 0.05] = 0.0
        return ids, w

    z_ids = np.arange(lo, dtype=np.uint32)
    z_w = np.array([1.0, 2.0 ** -24] + [2.0 ** -54] * (lo - 2))
    q_ids, q_w = vec(130)
    q = np.concatenate([z_ids, q_ids]), np.concatenate([z_w, q_w])
    return n_words, q, [vec(n) for n in (150, 129, 100, 65, 140)] + [(z_ids, z_w)]


def stale_score_fixture():
    """Query A scores X (id 2). In query B, X shares one word and fails the gate but is a neighbour
    of the scored keyframe 0, so 0's accumulated score includes X's score from A and pushes keyframe
    1 below 0.75 * best. -> (n_words, bows {id: bow}, neighbours {id: [ids]}, query A, query B)."""
    n_words = 64
    u = lambda ids: (np.array(ids, np.uint32), np.full(len(ids), 1.0 / len(ids)))   # noqa: E731
    bows = {0: u(list(range(0, 10))), 1: u(list(range(0, 9)) + [20]), 2: u([9] + list(range(30, 39)))}
    neighbours = {0: [2]}
    qa = u([9] + list(range(30, 39)))          # X itself: scored, mRelocScore = 1
    qb = u(list(range(0, 10)))                 # 0: 10 words, 1: 9 words, X: 1 word (gate: > 8)
    return n_words, bows, neighbours, qa, qb
