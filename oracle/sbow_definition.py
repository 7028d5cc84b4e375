"""SearchByBoW by definition: the reference's two forms restated in plain Python with np.float32
scalars, one source line per rule, written from the reference text. Test infrastructure only (as the
other *_definition modules): slow, sequential, and with tracing on it says which rule decided every
keyframe feature.

  SearchByBoW(KeyFrame*, Frame&, ...)        ORBmatcher.cc:223-425   -> py_sbow_kf_f
  SearchByBoW(KeyFrame*, KeyFrame*, ...)     ORBmatcher.cc:765-903   -> py_sbow_kf_kf
  rotation bin, ComputeThreeMaxima                                   -> sbp_definition.py_rot_bin, three_maxima_inds

A FeatureVector is given as (node_ids ascending, offsets, indices), the flattened std::map the C-ABI
takes; a node's indices keep the order of its std::vector. MapPoint* values are int32 handles, -1 for
NULL or isBad(). Angles are the `angle` fields of the keypoints the reference reads (mvKeysUn for a
single-camera keyframe or frame; mvKeys ++ mvKeysRight for two cameras).

Both functions return (nmatches, slots, trace):
  trace["nodes"]      the node ids the lower_bound walk found on both sides, in order
  trace["kf"][i]      for every keyframe feature of such a node (KF1 feature in the KF-KF form), keyed by
                      its index: {"node", "skip": None | "mp" | "right", "bd1", "bd2", "best", "rule",
                      "bin"} and, KF-F only, {"bd1R", "bd2R", "bestR", "ruleR", "binR"}
  rule                "none" (no free candidate), "distance", "ratio", "accepted"; after the histogram
                      an accepted entry of a dropped bin reads "dropped bin"
  ruleR               None (single camera, or no free right candidate), "left distance" (the right side
                      is looked at only inside bestDist1 <= TH_LOW), "distance", "accepted" / "dropped bin"
  trace["bins"]       the 30 bin counts and trace["kept_bins"] the kept bins (checkOri), else None
double=True evaluates the ratio test with mfNNratio as the double the caller wrote (the member is a
float), the rotation bin as rot / 30 in double and the 0.1f of ComputeThreeMaxima as a double: what a
careless restatement computes. The tests use it to prove that a planted case tells the two apart.
"""
from bisect import bisect_left

import numpy as np

from oracle.sbp_definition import HISTO_LENGTH, py_rot_bin, three_maxima_inds

f32 = np.float32
TH_LOW = 50   # ORBmatcher.cc:34


def _ham(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def ratio_passes(bd1, bd2, nnratio, double=False):
    """static_cast<float>(bestDist1) < mfNNratio * static_cast<float>(bestDist2) (ORBmatcher.cc:329, :850)."""
    if double:
        return bd1 < float(nnratio) * bd2
    return bool(f32(bd1) < f32(f32(nnratio) * f32(bd2)))


def _nodes(fv):
    ids = [int(v) for v in fv.node_ids]
    off = [int(v) for v in fv.offsets]
    return ids, [[int(v) for v in fv.indices[off[k]:off[k + 1]]] for k in range(len(ids))]


def _walk(ids_a, ids_b):
    """The while loop of ORBmatcher.cc:244-402 / :793-882 -> [(position in a, position in b)]."""
    a = b = 0
    out = []
    while a != len(ids_a) and b != len(ids_b):
        if ids_a[a] == ids_b[b]:
            out.append((a, b))
            a += 1
            b += 1
        elif ids_a[a] < ids_b[b]:
            a = bisect_left(ids_a, ids_b[b])   # lower_bound
        else:
            b = bisect_left(ids_b, ids_a[a])
    return out


def _commit(rot_hist, slots, n, double):
    """ORBmatcher.cc:404-422 / :884-902: every entry of a bin that is not one of the three maxima clears
    its slot and counts down."""
    ind = three_maxima_inds([len(h) for h in rot_hist], double)
    for i in range(HISTO_LENGTH):
        if i in ind:
            continue
        for slot, rec, key in rot_hist[i]:
            slots[slot] = -1
            n -= 1
            rec[key] = "dropped bin"
    return n, set(ind)


def py_sbow_kf_f(kf_angle, kf_desc, kf_mp, kf_fv, f_angle, f_desc, f_fv, nleft, nnratio, check_ori,
                 double=False):
    """ORBmatcher.cc:223-425. nleft: F.Nleft, None or -1 for a single-camera frame. slots: int32 [F.N]."""
    two = nleft is not None and nleft >= 0
    slots = np.full(len(f_desc), -1, np.int32)                            # :227
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    ids_k, vec_k = _nodes(kf_fv)
    ids_f, vec_f = _nodes(f_fv)
    n = 0
    tr = {"nodes": [], "kf": {}, "bins": None, "kept_bins": None}
    for a, b in _walk(ids_k, ids_f):
        tr["nodes"].append(ids_k[a])
        for ikf in vec_k[a]:                                              # :251
            rec = {"node": ids_k[a], "skip": None, "bd1": 256, "bd2": 256, "best": -1, "rule": "none", "bin": None,
                   "bd1R": 256, "bd2R": 256, "bestR": -1, "ruleR": None, "binR": None}
            tr["kf"][ikf] = rec
            if kf_mp[ikf] < 0:                                            # :257-261
                rec["skip"] = "mp"
                continue
            bd1, best, bd2 = 256, -1, 256
            bd1r, bestr, bd2r = 256, -1, 256
            for i in vec_f[b]:                                            # :273
                if slots[i] >= 0:                                         # :278 / :299
                    continue
                d = _ham(kf_desc[ikf], f_desc[i])
                if not two or i < nleft:                                  # :285-294 / :306-313
                    if d < bd1:
                        bd2, bd1, best = bd1, d, i
                    elif d < bd2:
                        bd2 = d
                else:                                                     # :315-322
                    if d < bd1r:
                        bd2r, bd1r, bestr = bd1r, d, i
                    elif d < bd2r:
                        bd2r = d
            rec.update(bd1=bd1, bd2=bd2, best=best, bd1R=bd1r, bd2R=bd2r, bestR=bestr)
            if best >= 0:
                rec["rule"] = "distance"
            if two and bestr >= 0:
                rec["ruleR"] = "left distance"
            if bd1 <= TH_LOW:                                             # :327
                if ratio_passes(bd1, bd2, nnratio, double):               # :329
                    slots[best] = kf_mp[ikf]
                    rec["rule"] = "accepted"
                    if check_ori:                                         # :338-353
                        rec["bin"] = py_rot_bin(kf_angle[ikf], f_angle[best], double)
                        rot_hist[rec["bin"]].append((best, rec, "rule"))
                    n += 1
                else:
                    rec["rule"] = "ratio"
                if two and bestr >= 0:
                    rec["ruleR"] = "distance"
                if bd1r <= TH_LOW:                                        # :357, the ratio test "|| true" (:359)
                    slots[bestr] = kf_mp[ikf]
                    rec["ruleR"] = "accepted"
                    if check_ori:                                         # :368-383
                        rec["binR"] = py_rot_bin(kf_angle[ikf], f_angle[bestr], double)
                        rot_hist[rec["binR"]].append((bestr, rec, "ruleR"))
                    n += 1
    if check_ori:                                                         # :404-422
        tr["bins"] = [len(h) for h in rot_hist]
        n, tr["kept_bins"] = _commit(rot_hist, slots, n, double)
    return n, slots, tr


def py_sbow_kf_kf(angle1, desc1, mp1, fv1, nleft1, angle2, desc2, mp2, fv2, nleft2, nnratio, check_ori,
                  double=False):
    """ORBmatcher.cc:765-903. nleft1 / nleft2: NLeft of a two-camera keyframe (mvKeysUn.size(): the indices
    from there on are skipped, :800-802, :820-822), None or -1 otherwise. slots: int32 [len(mp1)], KF2 handles."""
    lim1 = len(mp1) if nleft1 is None or nleft1 < 0 else nleft1
    lim2 = len(mp2) if nleft2 is None or nleft2 < 0 else nleft2
    slots = np.full(len(mp1), -1, np.int32)                               # :777
    matched2 = np.zeros(len(mp2), bool)                                   # :778
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    ids1, vec1 = _nodes(fv1)
    ids2, vec2 = _nodes(fv2)
    n = 0
    tr = {"nodes": [], "kf": {}, "bins": None, "kept_bins": None}
    for a, b in _walk(ids1, ids2):
        tr["nodes"].append(ids1[a])
        for i1 in vec1[a]:                                                # :797
            rec = {"node": ids1[a], "skip": None, "bd1": 256, "bd2": 256, "best": -1, "rule": "none", "bin": None}
            tr["kf"][i1] = rec
            if i1 >= lim1:                                                # :800-802
                rec["skip"] = "right"
                continue
            if mp1[i1] < 0:                                               # :804-808
                rec["skip"] = "mp"
                continue
            bd1, best, bd2 = 256, -1, 256
            for i2 in vec2[b]:                                            # :816
                if i2 >= lim2:                                            # :820-822
                    continue
                if matched2[i2] or mp2[i2] < 0:                           # :826-830
                    continue
                d = _ham(desc1[i1], desc2[i2])
                if d < bd1:                                               # :836-845
                    bd2, bd1, best = bd1, d, i2
                elif d < bd2:
                    bd2 = d
            rec.update(bd1=bd1, bd2=bd2, best=best)
            if best >= 0:
                rec["rule"] = "distance"
            if bd1 < TH_LOW:                                              # :848, strict
                if ratio_passes(bd1, bd2, nnratio, double):               # :850
                    slots[i1] = mp2[best]
                    matched2[best] = True
                    rec["rule"] = "accepted"
                    if check_ori:                                         # :855-865
                        rec["bin"] = py_rot_bin(angle1[i1], angle2[best], double)
                        rot_hist[rec["bin"]].append((i1, rec, "rule"))
                    n += 1
                else:
                    rec["rule"] = "ratio"
    if check_ori:                                                         # :884-902
        tr["bins"] = [len(h) for h in rot_hist]
        n, tr["kept_bins"] = _commit(rot_hist, slots, n, double)
    return n, slots, tr
