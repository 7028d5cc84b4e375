"""TemplatedVocabulary<FORB>::transform by definition: the reference's loops restated in plain Python, one
source line per rule, written from the reference text. Test infrastructure only (as the other *_definition
modules): slow, sequential, and the trace says which rule decided every feature, word and sum.

  transform(features, v, fv, levelsup)        TemplatedVocabulary.h:1139-1206   -> py_transform
  transform(feature, id, weight, nid, lup)    TemplatedVocabulary.h:1229-1270   -> descend
  loadFromBinFile                             TemplatedVocabulary.h:1478-1545   -> parse_bin
  BowVector::addWeight / addIfNotExist / normalize   BowVector.cpp:34-84
  FeatureVector::addFeature                   FeatureVector.cpp
  mustNormalize                               ScoringObject.h:74-89 (L1 for every scoring but L2_NORM,
                                              which takes L2, and DOT_PRODUCT, which does not normalise)
  Node(): word_id(0), isLeaf() = children.empty()    TemplatedVocabulary.h:328-340

A Python float is an IEEE double, so an explicit left-to-right `+=` loop gives the reference's bytes, and
so do `/`, abs and math.sqrt. No numpy reduction touches a weight.

py_transform takes the arrays ORBVocabulary.from_arrays takes and returns, in the oracle's layout,
((word ids uint32, weights float64), (node ids uint32, offsets int32 [nf + 1], indices uint32), trace):
  trace["f"][i]   per feature {"path": [node ids below the root], "levels": [{"node", "children", "dist",
                  "won" (index into children), "tie" (another child at the winning distance)}, ...],
                  "leaf", "word", "weight", "kept" (weight > 0), "nid", "nid_unset"}
                  (features with equal bytes share one record)
  trace["words"]  {word id: [addends in the order addWeight received them]} (IDF / BINARY: every weight
                  offered; the first is the one kept)
  trace["norm"]   the norm's addends in ascending word order (None where nothing is normalised)
order= sums those addend lists in another order than the reference's: "feature" (the reference's: left to
right), "sorted" (ascending by value, then left to right) or "pairwise" (a balanced tree). The tests use
it to prove that a planted case tells the orders apart.

The nid of a feature whose leaf lies above level L - levelsup: the reference's `NodeId nid` is an
uninitialised local that transform() never assigns on such a walk, so the reference gives no answer. This
project's rule is 0 (as both kernels and the oracle do); the trace marks the feature "nid_unset". That is
the project's rule, not the reference's.
"""
import math
import struct

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5
ORDERS = ("feature", "sorted", "pairwise")


def _bits(d):
    return int.from_bytes(bytes(d), "little")


def _ham(a, b):
    return bin(a ^ b).count("1")                                           # FORB::distance


def _pairwise(xs):
    if len(xs) == 1:
        return xs[0]
    h = len(xs) // 2
    return _pairwise(xs[:h]) + _pairwise(xs[h:])


def chain(addends, order="feature", start=None):
    """The sum of addends in the named order. start: the accumulator's initial value (the norm's 0.0);
    None: the first addend starts the chain (addWeight's insert, then +=)."""
    xs = [float(a) for a in addends]
    if order == "sorted":
        xs = sorted(xs)
    elif order == "pairwise":
        if not xs:
            return start
        s = _pairwise(xs)
        return s if start is None else start + s
    elif order != "feature":
        raise ValueError(order)
    if start is None:
        s, xs = xs[0], xs[1:]
    else:
        s = start
    for a in xs:
        s += a
    return s


class Tree:
    """m_nodes / m_words as loadFromBinFile leaves them (children in insertion order)."""

    def __init__(self, parents, is_leaf, desc, weights):
        n = len(parents)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        self.children = [[] for _ in range(n)]
        self.word_id = [0] * n                                             # Node(): word_id(0)
        self.weight = [float(w) for w in np.asarray(weights, np.float64)]
        self.desc = [_bits(desc[i]) for i in range(n)]
        self.n_words = 0
        for nid in range(1, n):
            self.children[int(parents[nid])].append(nid)                   # :1527
            if int(is_leaf[nid]) > 0:                                      # :1537
                self.word_id[nid] = self.n_words                           # :1539-1541
                self.n_words += 1


def parse_bin(data):
    """loadFromBinFile on the file's bytes -> (k, L, scoring, weighting, parents, is_leaf, desc, weights),
    None where the reference returns false. Nodes are read while the stream has data and fewer than
    expected_nodes exist (:1519), so bytes behind that count are never looked at."""
    k, L, n1, n2 = struct.unpack_from("<4i", data, 0)                       # :1495-1499
    if k < 0 or k > 20 or L < 1 or L > 10 or n1 < 0 or n1 > 5 or n2 < 0 or n2 > 3:   # :1501
        return None
    expected = int((math.pow(float(k), float(L) + 1) - 1) / (k - 1))       # :1512
    par, leaf, desc, w = [0], [0], [bytes(32)], [0.0]
    pos = 16
    while pos + 45 <= len(data) and len(par) < expected:                   # :1519
        pid, lf = struct.unpack_from("<iB", data, pos)
        par.append(pid)
        leaf.append(lf)
        desc.append(bytes(data[pos + 5:pos + 37]))
        w.append(struct.unpack_from("<d", data, pos + 37)[0])
        pos += 45
    d = np.frombuffer(b"".join(desc), np.uint8).reshape(-1, 32).copy()
    return k, L, n1, n2, np.array(par, np.int32), np.array(leaf, np.uint8), d, np.array(w, np.float64)


def descend(tree, L, feature, levelsup):
    """transform(feature, word_id, weight, nid, levelsup), :1229-1270 -> the feature's trace record."""
    nid_level = L - levelsup                                               # :1238
    nid, unset = 0, True
    if nid_level <= 0:                                                     # :1239
        nid, unset = 0, False
    final_id, current_level = 0, 0                                         # :1241-1242
    path, levels = [], []
    while True:                                                            # do
        current_level += 1                                                 # :1246
        nodes = tree.children[final_id]                                    # :1247
        parent = final_id
        final_id, won = nodes[0], 0                                        # :1248
        dist = [_ham(feature, tree.desc[c]) for c in nodes]
        best_d = dist[0]                                                   # :1250
        for j in range(1, len(nodes)):                                     # :1252
            if dist[j] < best_d:                                           # :1256, strict: the first of equals stays
                best_d, final_id, won = dist[j], nodes[j], j
        path.append(final_id)
        levels.append({"node": parent, "children": list(nodes), "dist": dist, "won": won,
                       "tie": dist.count(best_d) > 1})
        if current_level == nid_level:                                     # :1263
            nid, unset = final_id, False
        if not tree.children[final_id]:                                    # :1266 while(!isLeaf())
            break
    return {"path": path, "levels": levels, "leaf": final_id, "word": tree.word_id[final_id],   # :1269
            "weight": tree.weight[final_id], "kept": tree.weight[final_id] > 0,                 # :1270, :1169
            "nid": nid, "nid_unset": unset}


def py_transform(k, L, scoring, weighting, parents, is_leaf, desc, weights, features, levelsup=4, order="feature"):
    """TemplatedVocabulary.h:1139-1206. k is not read: a node has the children its `parents` give it."""
    if order not in ORDERS:
        raise ValueError(order)
    tree = Tree(parents, is_leaf, desc, weights)
    features = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
    tr = {"f": [], "words": {}, "norm": None}
    empty = ((np.zeros(0, np.uint32), np.zeros(0, np.float64)),
             (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)), tr)
    if tree.n_words == 0:                                                  # :1146 empty()
        return empty
    must, l1 = True, True                                                  # ScoringObject.h:74-89
    if scoring == L2_NORM:
        l1 = False
    if scoring == DOT_PRODUCT:
        must = False
    tf = weighting in (TF, TF_IDF)                                         # :1157
    v, fv, seen = {}, {}, {}
    for i in range(len(features)):                                         # :1160 / :1188
        key = features[i].tobytes()
        rec = seen.get(key)
        if rec is None:
            rec = seen[key] = descend(tree, L, _bits(features[i]), levelsup)   # :1167 / :1195
        tr["f"].append(rec)
        if rec["weight"] > 0:                                              # :1169 / :1197 not stopped (false for NaN)
            v.setdefault(rec["word"], []).append(rec["weight"])            # addWeight / addIfNotExist
            fv.setdefault(rec["nid"], []).append(i)                        # addFeature
    tr["words"] = {w: list(a) for w, a in v.items()}
    ids = sorted(v)                                                        # std::map: ascending word ids
    if tf:
        val = [chain(v[w], order) for w in ids]                            # addWeight: insert, then += in feature order
        if ids and not must:                                               # :1176
            nd = float(len(ids))                                           # :1179 v.size()
            val = [x / nd for x in val]                                    # :1181
    else:
        val = [v[w][0] for w in ids]                                       # addIfNotExist keeps the first
    if must:                                                               # :1205 BowVector::normalize
        add = [abs(x) for x in val] if l1 else [x * x for x in val]        # BowVector.cpp:70 / :75
        tr["norm"] = add
        norm = chain(add, order, start=0.0)
        if not l1:
            norm = math.sqrt(norm)                                         # :76
        if norm > 0.0:                                                     # :79
            val = [x / norm for x in val]
    nodes = sorted(fv)
    off = [0]
    for nd_ in nodes:
        off.append(off[-1] + len(fv[nd_]))
    idx = [i for nd_ in nodes for i in fv[nd_]]
    return ((np.array(ids, np.uint32), np.array(val, np.float64)),
            (np.array(nodes, np.uint32), np.array(off, np.int32), np.array(idx, np.uint32)), tr)
