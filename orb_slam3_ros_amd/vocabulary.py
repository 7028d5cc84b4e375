"""ORBVocabulary — host mirror of DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>
(Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h, typedef'd as ORB_SLAM3::ORBVocabulary) over the
C-ABI: loadFromBinFile and transform(features, BowVector, FeatureVector, levelsup), the call of
Frame::ComputeBoW. The tree lives in HBM; transform runs in liborbfe.so's HIP kernels.
Also writes the binary format (saveToBinFile layout) for synthetic vocabularies.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from . import _lib
from .matcher import FeatureVector

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5


def save_bin(k, L, scoring, weighting, parents, is_leaf, desc, weights) -> bytes:
    """TemplatedVocabulary::saveToBinFile layout: int k, L, scoring, weighting; then per node
    1..n-1: int parent, uchar isLeaf, uchar desc[32], double weight."""
    out = [struct.pack("<4i", k, L, scoring, weighting)]
    for i in range(1, len(parents)):
        out.append(struct.pack("<iB", int(parents[i]), int(is_leaf[i])) + bytes(desc[i]) +
                   struct.pack("<d", float(weights[i])))
    return b"".join(out)


class BowBatch:
    """The device result of ORBVocabulary.transform_batch (struct orbfe_bow_batch): per image a row of
    BowVector word ids / weights and of FeatureVector node ids / offsets / indices, and
    counts[i] = (bow_n, fv_n), (-1, -1) for an image whose input count was outside [0, cap]."""

    def __init__(self, nimg: int, cap: int, device):
        import torch as t
        self.nimg, self.cap = int(nimg), int(cap)
        self.voc = None   # the ORBVocabulary whose transform_batch filled it last
        self.bow_word_ids = t.zeros((nimg, cap), dtype=t.int32, device=device)   # u32 bit patterns
        self.bow_weights = t.zeros((nimg, cap), dtype=t.float64, device=device)
        self.fv_node_ids = t.zeros((nimg, cap), dtype=t.int32, device=device)
        self.fv_offsets = t.zeros((nimg, cap + 1), dtype=t.int32, device=device)
        self.fv_indices = t.zeros((nimg, cap), dtype=t.int32, device=device)
        self.counts = t.zeros((nimg, 2), dtype=t.int32, device=device)
        self.c = _lib.BowBatchStruct(self.bow_word_ids.data_ptr(), self.bow_weights.data_ptr(),
                                     self.fv_node_ids.data_ptr(), self.fv_offsets.data_ptr(),
                                     self.fv_indices.data_ptr(), self.counts.data_ptr())

    def ref(self):
        return ctypes.byref(self.c)

    def host(self, i: int):
        """Image i copied to the host (synchronises): ((word ids, weights), FeatureVector), the shape of
        ORBVocabulary.transform."""
        nb, nf = (int(v) for v in self.counts[i].cpu().numpy())
        if nb < 0:
            raise _lib.OrbfeError(f"image {i} of the batch had a count outside [0, cap]")
        ids = self.bow_word_ids[i, :nb].cpu().numpy().view(np.uint32).copy()
        w = self.bow_weights[i, :nb].cpu().numpy().copy()
        fid = self.fv_node_ids[i, :nf].cpu().numpy().view(np.uint32)
        foff = self.fv_offsets[i, :nf + 1].cpu().numpy()
        fidx = self.fv_indices[i, :int(foff[nf]) if nf else 0].cpu().numpy().view(np.uint32)
        fv = FeatureVector({int(fid[k]): fidx[foff[k]:foff[k + 1]].tolist() for k in range(nf)})
        return (ids, w), fv

    def host_feature_vector(self, i: int):
        """Image i's FeatureVector alone, copied to the host (synchronises); the BowVector stays in HBM."""
        nf = int(self.counts[i, 1].cpu())
        if nf < 0:
            raise _lib.OrbfeError(f"image {i} of the batch had a count outside [0, cap]")
        fid = self.fv_node_ids[i, :nf].cpu().numpy().view(np.uint32)
        foff = self.fv_offsets[i, :nf + 1].cpu().numpy()
        fidx = self.fv_indices[i, :int(foff[nf]) if nf else 0].cpu().numpy().view(np.uint32)
        return FeatureVector({int(fid[k]): fidx[foff[k]:foff[k + 1]].tolist() for k in range(nf)})


class ORBVocabulary:
    def __init__(self, handle, lib):
        self._h = handle
        self._lib = lib
        k, L, nn, nw = (ctypes.c_int32() for _ in range(4))
        _lib.check(lib.orbfe_vocabulary_info(handle, ctypes.byref(k), ctypes.byref(L), ctypes.byref(nn),
                                             ctypes.byref(nw)), "vocabulary_info")
        self.k, self.L, self.n_nodes, self.n_words = k.value, L.value, nn.value, nw.value

    @classmethod
    def from_bin(cls, data: bytes):
        """loadFromBinFile from the file's bytes."""
        lib = _lib.load()
        h = ctypes.c_void_p()
        buf = np.frombuffer(data, np.uint8)
        _lib.check(lib.orbfe_vocabulary_load_bin(buf.ctypes.data, len(buf), ctypes.byref(h)), "vocabulary_load_bin")
        return cls(h, lib)

    @classmethod
    def from_arrays(cls, k, L, scoring, weighting, parents, is_leaf, desc, weights):
        lib = _lib.load()
        h = ctypes.c_void_p()
        par = np.ascontiguousarray(parents, np.int32)
        leaf = np.ascontiguousarray(is_leaf, np.uint8)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        w = np.ascontiguousarray(weights, np.float64)
        _lib.check(lib.orbfe_vocabulary_create(k, L, scoring, weighting, len(par), par.ctypes.data, leaf.ctypes.data,
                                               d.ctypes.data, w.ctypes.data, ctypes.byref(h)), "vocabulary_create")
        return cls(h, lib)

    def transform(self, desc, levelsup: int = 4):
        """-> (BowVector as (word ids, weights), FeatureVector)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        bid = np.zeros(max(n, 1), np.uint32)
        bw = np.zeros(max(n, 1), np.float64)
        fid = np.zeros(max(n, 1), np.uint32)
        foff = np.zeros(n + 1, np.int32)
        fidx = np.zeros(max(n, 1), np.uint32)
        nb, nf = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self._lib.orbfe_vocabulary_transform(self._h, d.ctypes.data, n, int(levelsup), bid.ctypes.data,
                                                        bw.ctypes.data, ctypes.byref(nb), fid.ctypes.data,
                                                        foff.ctypes.data, fidx.ctypes.data, ctypes.byref(nf)),
                   "vocabulary_transform")
        nb, nf = nb.value, nf.value
        fv = FeatureVector({int(fid[i]): fidx[foff[i]:foff[i + 1]].tolist() for i in range(nf)})
        return (bid[:nb].copy(), bw[:nb].copy()), fv

    def transform_batch(self, desc, counts, levelsup: int = 4, out=None, stream=None):
        """transform for every image of a device batch, stream-ordered and without a host wait.
        desc: uint8 [nimg, cap, 32] and counts: int32 [nimg] or [nimg, s] (image i's count is
        counts[i, 0]; the extractor's [nimg, 2] batch counts fit), contiguous torch device tensors.
        out: a BowBatch to fill again (same nimg and cap); stream: a hipStream_t, default the current
        torch stream. -> BowBatch (device tensors; BowBatch.host(i) copies one image back)."""
        import torch
        if not (desc.is_cuda and desc.dtype == torch.uint8 and desc.dim() == 3 and desc.shape[2] == 32 and
                desc.is_contiguous()):
            raise ValueError("desc: a contiguous uint8 [nimg, cap, 32] device tensor")
        nimg, cap = int(desc.shape[0]), int(desc.shape[1])
        if not (counts.is_cuda and counts.dtype == torch.int32 and counts.dim() in (1, 2) and
                counts.shape[0] == nimg and counts.is_contiguous()):
            raise ValueError("counts: a contiguous int32 [nimg] or [nimg, s] device tensor")
        stride = 1 if counts.dim() == 1 else int(counts.shape[1])
        if out is None:
            out = BowBatch(nimg, cap, desc.device)
        elif (out.nimg, out.cap) != (nimg, cap):
            raise ValueError("out was made for another batch shape")
        if stream is None:
            stream = torch.cuda.current_stream(desc.device).cuda_stream
        _lib.check(self._lib.orbfe_vocabulary_transform_batch(self._h, desc.data_ptr(), counts.data_ptr(), stride, nimg,
                                                              cap, int(levelsup), out.ref(), stream),
                   "vocabulary_transform_batch")
        out.voc = self
        return out

    def compute_bow(self, F, levelsup: int = 4):
        """Frame::ComputeBoW for a MatchFrame, a DeviceMatchFrame or a device view
        (matcher.current_frame_view): -> (BowVector as (word ids, weights), FeatureVector). The
        descriptors of the device forms are read in HBM."""
        from .matcher import CFrame, DeviceMatchFrame
        ref = F.ref()
        if isinstance(F, DeviceMatchFrame):   # its struct carries device pointers without the flag
            c = CFrame()
            ctypes.memmove(ctypes.byref(c), F.ref(), ctypes.sizeof(CFrame))
            c.device = 1
            ref = ctypes.byref(c)
        n = int(F.N)
        bid = np.zeros(max(n, 1), np.uint32)
        bw = np.zeros(max(n, 1), np.float64)
        fid = np.zeros(max(n, 1), np.uint32)
        foff = np.zeros(n + 1, np.int32)
        fidx = np.zeros(max(n, 1), np.uint32)
        nb, nf = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self._lib.orbfe_frame_compute_bow(self._h, ref, int(levelsup), bid.ctypes.data, bw.ctypes.data,
                                                     ctypes.byref(nb), fid.ctypes.data, foff.ctypes.data,
                                                     fidx.ctypes.data, ctypes.byref(nf)), "frame_compute_bow")
        nb, nf = nb.value, nf.value
        fv = FeatureVector({int(fid[i]): fidx[foff[i]:foff[i + 1]].tolist() for i in range(nf)})
        return (bid[:nb].copy(), bw[:nb].copy()), fv

    def close(self):
        if self._h:
            self._lib.orbfe_vocabulary_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth_vocabulary(rng, k: int = 10, L: int = 4, stop_frac: float = 0.02):
    """A full k-ary tree of depth L in DBoW2's node order (breadth-first, children consecutive) with
    random descriptors; leaf weights are idf-like positive values, a few 0 (stopped words)."""
    parents = [0]
    is_leaf = [0]
    level_nodes = [0]
    for lv in range(1, L + 1):
        nxt = []
        for p in level_nodes:
            for _ in range(k):
                parents.append(p)
                is_leaf.append(1 if lv == L else 0)
                nxt.append(len(parents) - 1)
        level_nodes = nxt
    n = len(parents)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    w = rng.uniform(0.1, 6.0, n)
    w[rng.random(n) < stop_frac] = 0.0
    w[0] = 0.0
    return np.array(parents, np.int32), np.array(is_leaf, np.uint8), desc, w
