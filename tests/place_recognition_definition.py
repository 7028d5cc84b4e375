"""TEST INFRASTRUCTURE (CPU only): a literal restatement of KeyFrameDatabase::DetectNBestCandidates
(KeyFrameDatabase.cc:604-730) over tests/kfdb_definition.py's inverted file. The per-keyframe state
(mnPlaceRecognitionQuery, mnPlaceRecognitionWords, mPlaceRecognitionScore) persists between queries
and is apart from the relocalisation state; Python float is the reference's double and np.float32
every float variable of the reference.

Two documented departures, shared with orbfe_kfdb_detect_nbest: every call is a fresh query (the
stamp is a query serial, not pKF->mnId), and the isBad() branch of the selection walk has no
counterpart (a bad keyframe has been erased)."""
import numpy as np

from kfdb_definition import F32, KF, KeyFrameDatabaseDef, l1_score


class PlaceRecognitionDef(KeyFrameDatabaseDef):
    def __init__(self, n_words):
        super().__init__(n_words)
        self.next_place_query = 0

    def add(self, kf):
        kf.mnPlaceRecognitionQuery = -1
        kf.mnPlaceRecognitionWords = 0
        kf.mPlaceRecognitionScore = F32(0)   # a new entry starts from 0
        super().add(kf)

    def DetectNBestCandidates(self, bow, connected, map_id=0, n=3, bad_maps=()):
        """bow: pKF->mBowVec; connected: ids of pKF->GetConnectedKeyFrames() -> (loop ids, merge ids)."""
        q_ids = [int(x) for x in bow[0]]
        q_w = [float(x) for x in bow[1]]
        qid = self.next_place_query
        self.next_place_query += 1
        spConnectedKF = {int(c) for c in connected}
        lKFsSharingWords = []
        for w in q_ids:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnPlaceRecognitionQuery != qid:
                    pKFi.mnPlaceRecognitionWords = 0
                    if pKFi.mnId not in spConnectedKF:
                        pKFi.mnPlaceRecognitionQuery = qid
                        lKFsSharingWords.append(pKFi)
                pKFi.mnPlaceRecognitionWords += 1
        empty = (np.zeros(0, np.int32), np.zeros(0, np.int32))
        if not lKFsSharingWords:
            return empty
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnPlaceRecognitionWords > maxCommonWords:
                maxCommonWords = pKFi.mnPlaceRecognitionWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnPlaceRecognitionWords > minCommonWords:
                si = F32(l1_score(q_ids, q_w, pKFi.words, pKFi.weights))
                pKFi.mPlaceRecognitionScore = si
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return empty
        lAccScoreAndMatch = []
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for nb in pKFi.neighbours[:10]:
                pKF2 = self._resolve(nb)
                if pKF2 is None or pKF2.mnPlaceRecognitionQuery != qid:
                    continue
                accScore = F32(accScore + pKF2.mPlaceRecognitionScore)
                if pKF2.mPlaceRecognitionScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mPlaceRecognitionScore
            lAccScoreAndMatch.append((accScore, pBestKF))
        # std::list::sort(compFirst): a stable merge sort, a.first > b.first
        lAccScoreAndMatch = sorted(lAccScoreAndMatch, key=lambda p: -float(p[0]))
        vpLoopCand, vpMergeCand = [], []
        spAlreadyAddedKF = set()
        i = 0
        while i < len(lAccScoreAndMatch) and (len(vpLoopCand) < n or len(vpMergeCand) < n):
            pKFi = lAccScoreAndMatch[i][1]
            if id(pKFi) not in spAlreadyAddedKF:
                if map_id == pKFi.map_id and len(vpLoopCand) < n:
                    vpLoopCand.append(pKFi.mnId)
                elif map_id != pKFi.map_id and len(vpMergeCand) < n and pKFi.map_id not in bad_maps:
                    vpMergeCand.append(pKFi.mnId)
                spAlreadyAddedKF.add(id(pKFi))
            i += 1
        return np.array(vpLoopCand, np.int32), np.array(vpMergeCand, np.int32)


# ---- fixtures shared by tests/test_place_recognition_definition.py and tests/test_gpu_kfdb_nbest.py ----

def uniform(ids):
    return np.array(ids, np.uint32), np.full(len(ids), 1.0 / len(ids))


def gate_fixture():
    """Keyframe 0 shares all 10 query words, 1 shares 8, 2 shares 7. With 0 in the list the gate is
    int(10 * 0.8f) = 8 and only 0 is scored; with 0 connected the maximum is 8, the gate 6, and 1 and 2
    are both scored. -> (n_words, bows {id: bow}, query)."""
    bows = {0: uniform(range(0, 10)), 1: uniform(list(range(0, 8)) + [20, 21]),
            2: uniform(list(range(0, 7)) + [22, 23, 24])}
    return 64, bows, uniform(range(0, 10))


def tie_fixture():
    """Six keyframes with the same BowVector (equal scores, hence equal accScores without neighbours):
    the stable sort keeps the list order, which is the add order. Maps alternate 0, 1."""
    bows = {10 + k: uniform(range(0, 8)) for k in range(6)}
    maps = {10 + k: k % 2 for k in range(6)}
    return 64, bows, maps, uniform(range(0, 8))


def dedupe_fixture():
    """Keyframe 2 matches the query best. 0 and 1 match it worse and both have 2 as neighbour, so the
    entries of 0, 1 and 2 all name 2 as pBestKF: it is returned once. 3 matches worse still and has no
    neighbour. -> (n_words, bows, neighbours, query); expected loop ids [2, 3]."""
    q = uniform(range(0, 10))
    bows = {0: uniform(list(range(0, 9)) + [30]), 1: uniform(list(range(0, 9)) + [31]), 2: uniform(range(0, 10)),
            3: uniform(list(range(0, 9)) + [32, 33, 34])}
    return 64, bows, {0: [2], 1: [2]}, q


def stale_place_fixture():
    """Query A scores X (id 2). In query B, X shares one word and fails the gate, but it is a neighbour of
    keyframe 1, whose accumulated score therefore includes X's score from A: 1 sorts before 0 although 0
    alone matches B better. -> (n_words, bows, neighbours, query A, query B)."""
    bows = {0: uniform(range(0, 10)), 1: uniform(list(range(0, 9)) + [20]), 2: uniform([9] + list(range(30, 39)))}
    return 64, bows, {1: [2]}, uniform([9] + list(range(30, 39))), uniform(range(0, 10))


def random_scene(rng, n_words, n_kf, n_maps=2):
    """-> (bows, neighbours, maps) of n_kf keyframes: BowVectors of 10-40 words over n_words, up to 12
    neighbours each (more than 10 are cut; some name absent ids), n_maps maps."""
    from kfdb_definition import random_bow
    bows = {i: random_bow(rng, n_words, int(rng.integers(10, min(40, n_words)))) for i in range(n_kf)}
    neighbours = {i: [int(x) for x in rng.integers(0, n_kf + 5, int(rng.integers(0, 13)))] for i in range(n_kf)}
    maps = {i: int(rng.integers(0, n_maps)) for i in range(n_kf)}
    return bows, neighbours, maps


def build(db_cls, n_words, bows, neighbours=None, maps=None):
    db = db_cls(n_words)
    for i, b in bows.items():
        db.add(KF(i, b, (neighbours or {}).get(i, ()), (maps or {}).get(i, 0)))
    return db
