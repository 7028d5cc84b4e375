"""KeyFrameDatabase — host mirror of ORB_SLAM3::KeyFrameDatabase's relocalisation side
(KeyFrameDatabase.cc:39-77, :733-845) over the C-ABI (orbfe_kfdb_*). Every added keyframe's
BowVector lives in HBM; DetectRelocalizationCandidates scores the frame against all of them in
liborbfe.so's HIP kernel and runs the covisibility tail inside the library.
Keyframes are named by ids >= 0: indices into the caller's own keyframe table, the same table that
holds its KeyFrameFeatures for SearchByBoWBatch.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


def _bow(bow):
    ids, w = bow
    ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
    w = np.ascontiguousarray(w, np.float64).reshape(-1)
    if len(ids) != len(w):
        raise ValueError("a BowVector needs one weight per word id")
    return ids, w


def _lookup(table, kf_id, default):
    if table is None:
        return default
    if callable(table):
        return table(kf_id)
    return table.get(kf_id, default)


class KeyFrameDatabase:
    def __init__(self, n_words: int):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        _lib.check(self._lib.orbfe_kfdb_create(int(n_words), ctypes.byref(self._h)), "KeyFrameDatabase")
        self.n_words = int(n_words)

    def add(self, kf_id: int, bow) -> None:
        """bow: the (word_ids, weights) pair ORBVocabulary.transform returns (pKF->mBowVec)."""
        ids, w = _bow(bow)
        _lib.check(self._lib.orbfe_kfdb_add(self._h, int(kf_id), ids.ctypes.data, w.ctypes.data, len(ids)),
                   "KeyFrameDatabase.add")

    def add_batch(self, kf_ids, bow_batch, stream=None) -> None:
        """add() for the images of a vocabulary.BowBatch, device to device: image i becomes keyframe
        kf_ids[i] in array order, an id < 0 skips its image. The batch's vocabulary (the one whose
        transform_batch filled it) must have this database's word count. stream: the hipStream_t the
        batch was made on (default: the current torch stream); it is waited for. Refused as a whole
        (nothing added) when an id repeats or is present, or an image to add has counts (-1, -1)."""
        ids = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        if len(ids) != bow_batch.nimg:
            raise ValueError("add_batch needs one keyframe id per image of the batch")
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(bow_batch.counts.device).cuda_stream
        if bow_batch.voc is None:
            raise ValueError("the batch has not been filled by ORBVocabulary.transform_batch")
        _lib.check(self._lib.orbfe_kfdb_add_batch(self._h, bow_batch.voc._h, ids.ctypes.data, bow_batch.ref(), len(ids),
                                                  bow_batch.cap, stream), "KeyFrameDatabase.add_batch")

    def erase(self, kf_id: int) -> None:
        _lib.check(self._lib.orbfe_kfdb_erase(self._h, int(kf_id)), "KeyFrameDatabase.erase")

    def clear(self) -> None:
        _lib.check(self._lib.orbfe_kfdb_clear(self._h), "KeyFrameDatabase.clear")

    def __len__(self) -> int:
        return _lib.check(self._lib.orbfe_kfdb_size(self._h), "KeyFrameDatabase.size")

    def shared_words(self, bow):
        """-> (kf_ids, words, scores, scored, maxCommonWords): lKFsSharingWords in the reference's list
        order with mnRelocWords, and si (float32) where scored. Updates mRelocScore of the scored ones."""
        ids, w = _bow(bow)
        cap = max(len(self), 1)
        while True:   # the cap protocol: another thread may add between len() and the query
            kf = np.zeros(cap, np.int32)
            words = np.zeros(cap, np.int32)
            scores = np.zeros(cap, np.float32)
            scored = np.zeros(cap, np.uint8)
            n, mx = ctypes.c_int32(-1), ctypes.c_int32()
            rc = self._lib.orbfe_kfdb_shared_words(self._h, ids.ctypes.data, w.ctypes.data, len(ids), kf.ctypes.data,
                                                   words.ctypes.data, scores.ctypes.data, scored.ctypes.data, cap,
                                                   ctypes.byref(n), ctypes.byref(mx))
            if rc == _lib.ORBFE_E_ARG and n.value > cap:
                cap = n.value   # nothing was written and no state changed: ask again with the needed count
                continue
            break
        _lib.check(rc, "KeyFrameDatabase.shared_words")
        n = n.value
        return kf[:n].copy(), words[:n].copy(), scores[:n].copy(), scored[:n].astype(bool), mx.value

    def DetectRelocalizationCandidates(self, bow, map_id: int = 0, neighbours=None, maps=None) -> np.ndarray:
        """vpRelocCandidates as an int32 array of keyframe ids. neighbours: dict or callable
        kf_id -> GetBestCovisibilityKeyFrames(10) ids (more than 10 are cut); maps: dict or callable
        kf_id -> map id (missing: map_id). The callables must not use this database."""
        ids, w = _bow(bow)
        cap = max(len(self), 1)
        # ctypes swallows an exception raised inside a callback: record the first one and re-raise it
        # after the call, as SearchForTriangulationEpi does. After an error the callback answers -1, a
        # count the library refuses with ORBFE_E_ARG, so the failed call commits no mRelocScore.
        err = []

        def info(ctx, kf_id, nb, mp):
            mp[0] = int(map_id)
            if err:
                return -1
            try:
                mp[0] = int(_lookup(maps, kf_id, map_id))
                ns = list(_lookup(neighbours, kf_id, ()))[:10]
                for i, v in enumerate(ns):
                    nb[i] = int(v)
                return len(ns)
            except BaseException as ex:  # noqa: BLE001 - re-raised below
                err.append(ex)
                return -1

        cb = _lib.KF_INFO_FN(info) if (neighbours is not None or maps is not None) else _lib.KF_INFO_FN()
        while True:   # the cap protocol: another thread may add between len() and the query
            out = np.zeros(cap, np.int32)
            n = ctypes.c_int32(-1)
            rc = self._lib.orbfe_kfdb_detect_reloc(self._h, ids.ctypes.data, w.ctypes.data, len(ids), int(map_id), cb,
                                                   None, out.ctypes.data, cap, ctypes.byref(n))
            if err:
                raise err[0]
            if rc == _lib.ORBFE_E_ARG and n.value > cap:
                cap = n.value   # no state changed: ask again with the needed count
                continue
            break
        _lib.check(rc, "DetectRelocalizationCandidates")
        return out[:n.value].copy()

    def DetectNBestCandidates(self, bow, connected, map_id: int = 0, n: int = 3, neighbours=None, maps=None,
                              bad_maps=()):
        """DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, n) (KeyFrameDatabase.cc:604-730) ->
        (loop_ids, merge_ids), int32 arrays of at most n keyframe ids each. bow: pKF->mBowVec; connected:
        pKF->GetConnectedKeyFrames() as ids; map_id: pKF->GetMap(); neighbours / maps as for
        DetectRelocalizationCandidates; bad_maps: ids of the maps with IsBad()."""
        ids, w = _bow(bow)
        con = np.ascontiguousarray(list(connected), np.int32).reshape(-1)
        bad = np.ascontiguousarray(list(bad_maps), np.int32).reshape(-1)
        n = int(n)
        # the callback-error protocol of DetectRelocalizationCandidates
        err = []

        def info(ctx, kf_id, nb, mp):
            mp[0] = int(map_id)
            if err:
                return -1
            try:
                mp[0] = int(_lookup(maps, kf_id, map_id))
                ns = list(_lookup(neighbours, kf_id, ()))[:10]
                for i, v in enumerate(ns):
                    nb[i] = int(v)
                return len(ns)
            except BaseException as ex:  # noqa: BLE001 - re-raised below
                err.append(ex)
                return -1

        cb = _lib.KF_INFO_FN(info) if (neighbours is not None or maps is not None) else _lib.KF_INFO_FN()
        loop = np.zeros(max(n, 1), np.int32)
        merge = np.zeros(max(n, 1), np.int32)
        nl, nm = ctypes.c_int32(0), ctypes.c_int32(0)
        rc = self._lib.orbfe_kfdb_detect_nbest(self._h, ids.ctypes.data, w.ctypes.data, len(ids),
                                               con.ctypes.data if len(con) else None, len(con), int(map_id),
                                               bad.ctypes.data if len(bad) else None, len(bad), n, cb, None,
                                               loop.ctypes.data, ctypes.byref(nl), merge.ctypes.data, ctypes.byref(nm))
        if err:
            raise err[0]
        _lib.check(rc, "DetectNBestCandidates")
        return loop[:nl.value].copy(), merge[:nm.value].copy()

    def close(self) -> None:
        if self._h:
            self._lib.orbfe_kfdb_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
