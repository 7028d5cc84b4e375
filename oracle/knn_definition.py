"""Plain definition of the descriptor stage of Frame::ComputeStereoFishEyeMatches (Frame.cc:1126-1151):
BFMatcher(NORM_HAMMING).knnMatch(k = 2) of the lapping rows of the left image against those of the right,
then `(*it).size() >= 2 && (*it)[0].distance < (*it)[1].distance * 0.7`.

Written for reading, not speed: a left-to-right scan per query, one rule per line. The C++ oracle
(oro_stereo_knn_ratio) and the three kernels (k_knn2, k_knn2_batch<16>, k_knn2_batch<4>) must give the same
slots; tests/test_knn_definition.py holds the oracle to this file on every planted case of
tests/knn_patterns.py.

knnMatch keeps, per query, the two nearest train rows; of equally near rows the earlier one comes first
(strict-less insertion), so the best distance occurring twice gives d1 == d0 and the ratio test rejects.
DMatch distances are float and the reference multiplies by the double literal 0.7; the API here takes a
float ratio, so the rule is float32(d0) < double(float32(d1)) * double(float32(ratio)) ("kernel").
"""
import numpy as np

INF = 0x7FFFFFFF   # the distance of a missing neighbour (fewer than two train rows)
VARIANTS = ("kernel", "float", "literal")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(a, b):
    """Hamming distance of two 32-byte rows."""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    assert a.shape == (32,) and b.shape == (32,)
    return int(_POP[a ^ b].sum())


def distances(q, train):
    """hamming(q, train[j]) for every j, in one array."""
    train = np.asarray(train, np.uint8).reshape(-1, 32)
    return _POP[np.asarray(q, np.uint8)[None, :] ^ train].sum(1)


def top2_trace(q, train):
    """The scan of knnMatch(k = 2): (d0, d1, t0, t1). t1 is the row that holds the second place at the end
    (-1 when there is none)."""
    d0, d1, t0, t1 = INF, INF, -1, -1
    for j, d in enumerate(distances(q, train).tolist()):
        if d < d0:
            d1, t1 = d0, t0
            d0, t0 = d, j
        elif d < d1:
            d1, t1 = d, j
    return d0, d1, t0, t1


def top2(q, train):
    return top2_trace(q, train)[:3]


def ratio_passes(d0, d1, ratio, variant="kernel"):
    f32, f64 = np.float32, np.float64
    if variant == "kernel":    # the float ratio widened, the product in double
        return bool(f32(d0) < f64(f32(d1)) * f64(f32(ratio)))
    if variant == "float":     # the product rounded to float
        return bool(f32(d0) < f32(f32(d1) * f32(ratio)))
    if variant == "literal":   # the ratio as the double literal of the reference's `* 0.7`
        return bool(f32(d0) < f64(f32(d1)) * f64(ratio))
    raise ValueError(variant)


def knn_ratio(L, R, ratio, variant="kernel", trace=None):
    """(train [nl], dist [nl], ngood). trace, a list, receives per query (d0, d1, t0, t1, rule) with rule one
    of "few-train" (fewer than two train rows), "ratio-reject", "pass"."""
    L = np.asarray(L, np.uint8).reshape(-1, 32)
    R = np.asarray(R, np.uint8).reshape(-1, 32)
    train = np.full(len(L), -1, np.int32)
    dist = np.full(len(L), -1, np.int32)
    for i, q in enumerate(L):
        d0, d1, t0, t1 = top2_trace(q, R)
        if len(R) < 2:
            rule = "few-train"
        elif not ratio_passes(d0, d1, ratio, variant):
            rule = "ratio-reject"
        else:
            rule = "pass"
            train[i], dist[i] = t0, d0
        if trace is not None:
            trace.append((d0, d1, t0, t1, rule))
    return train, dist, int((train >= 0).sum())


def knn_frame(counts_l, desc_l, counts_r, desc_r, cap, ratio, variant="kernel", trace=None):
    """One frame of the batched form: counts = (n, monoIndex) of an image, desc its [cap][32] rows. Queries
    are rows [monoL, nL), train rows [monoR, nR). (l2r [cap], dist [cap], ngood) in full keypoint numbering."""
    nL, monoL = int(counts_l[0]), int(counts_l[1])
    nR, monoR = int(counts_r[0]), int(counts_r[1])
    desc_l = np.asarray(desc_l, np.uint8).reshape(cap, 32)
    desc_r = np.asarray(desc_r, np.uint8).reshape(cap, 32)
    l2r = np.full(cap, -1, np.int32)
    dist = np.full(cap, -1, np.int32)
    if nL > monoL:
        t, d, _ = knn_ratio(desc_l[monoL:nL], desc_r[monoR:max(nR, monoR)], ratio, variant, trace)
        l2r[monoL:nL] = np.where(t >= 0, t + monoR, -1)
        dist[monoL:nL] = d
    return l2r, dist, int((l2r >= 0).sum())
