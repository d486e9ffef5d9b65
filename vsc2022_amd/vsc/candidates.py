"""Candidate generation: host-side mirror of the reference's `vsc/candidates.py`
(same names and semantics; paths relative to /root/reference).

`CandidateGeneration.query` with the stock `MaxScoreAggregation` never builds per-hit Python
objects: the score-sorted hit list stays in HBM and libvscmi's vsc_pair_max produces the
(query video, ref video, max score) table directly.  So do the other built-in aggregations
(`SumScoreAggregation`, `MeanScoreAggregation`, `TopMeanScoreAggregation(m)`) and the k-NN
retrieval (`global_k < 0`) of all four, through vsc_index_candidates_agg.  Any SUBCLASS of them and
any user `ScoreAggregation` goes through the generic `VideoIndex.search` -> `PairMatches` route,
unchanged.

The built-in aggregations share one definition (include/vscmi.h, vsc_pair_aggregate): the pair's
fp32 hit scores as float64, sorted descending, added one by one from 0.0 in that order; the result
rounded to fp32.  Finite scores are a precondition.  `aggregate()` below is the host statement of
it, the kernels of csrc/pair_reduce.hip compute the same bits.
"""
import ctypes
import logging
from abc import ABC, abstractmethod
from collections.abc import Sequence
from typing import List

import numpy as np

from vsc2022_amd import _lib
from vsc2022_amd.vsc.index import KNN_WARNING, PairMatches, VideoFeature, VideoIndex, VideoLayout
from vsc2022_amd.vsc.metrics import CandidatePair


class ScoreAggregation(ABC):
    """vsc/candidates.py:14-21"""

    @abstractmethod
    def aggregate(self, match: PairMatches) -> float:
        pass

    def score(self, match: PairMatches) -> CandidatePair:
        score = self.aggregate(match)
        return CandidatePair(query_id=match.query_id, ref_id=match.ref_id, score=score)


class MaxScoreAggregation(ScoreAggregation):
    """vsc/candidates.py:24-26"""

    def aggregate(self, match: PairMatches) -> float:
        scores = getattr(match.matches, "scores", None)
        if scores is None:
            scores = [m.score for m in match.matches]
        return np.max(scores)


def _descending_chain(match: PairMatches) -> np.ndarray:
    """chain[k] = the float64 sum of the k best hit scores of a pair (fp32), added one by one from +0.0 in descending
    order: np.cumsum adds strictly left to right, and the leading 0.0 makes the first add `0.0 + d[0]` (a run of -0.0
    sums to +0.0, as in the kernel)."""
    scores = getattr(match.matches, "scores", None)
    if scores is None:
        scores = [m.score for m in match.matches]
    d = np.sort(np.asarray(scores, dtype=np.float32).astype(np.float64))[::-1]
    return np.cumsum(np.concatenate((np.zeros(1), d)))


def _f32(x) -> np.float32:
    """float64 -> fp32, round to nearest; a sum beyond the fp32 range becomes +-inf, as the kernel's conversion does."""
    with np.errstate(over="ignore"):
        return np.float32(x)


class SumScoreAggregation(ScoreAggregation):
    """Sum of the hit scores: float64 adds from 0.0 in descending score order."""

    def aggregate(self, match: PairMatches) -> float:
        return _f32(_descending_chain(match)[-1])


class MeanScoreAggregation(ScoreAggregation):
    """That sum over the number of hits."""

    def aggregate(self, match: PairMatches) -> float:
        chain = _descending_chain(match)
        return _f32(chain[-1] / np.float64(len(chain) - 1))


class TopMeanScoreAggregation(ScoreAggregation):
    """Mean of the m best hit scores (of all of them where the pair has fewer): m = 1 is the max."""

    def __init__(self, m: int):
        if int(m) != m or m < 1:
            raise ValueError(f"TopMeanScoreAggregation: m must be an integer >= 1, got {m!r}")
        self.m = int(m)

    def aggregate(self, match: PairMatches) -> float:
        chain = _descending_chain(match)
        k = min(self.m, len(chain) - 1)
        return _f32(chain[k] / np.float64(k))


def device_aggregation(aggregation):
    """(VSC_AGG_* id, top_m) of an aggregation that runs on the device, None for every other.  EXACT types only: a
    subclass may override `aggregate` or `score`, so it keeps the generic route."""
    t = type(aggregation)
    if t is MaxScoreAggregation:
        return _lib.AGG_MAX, 1
    if t is SumScoreAggregation:
        return _lib.AGG_SUM, 1
    if t is MeanScoreAggregation:
        return _lib.AGG_MEAN, 1
    if t is TopMeanScoreAggregation:
        return _lib.AGG_TOPMEAN, int(aggregation.m)
    return None


def device_route(aggregation, global_k: int, ntotal: int):
    """How `CandidateGeneration.query` runs: "max" (vsc_index_candidates, as ever), ("agg", id, top_m)
    (vsc_index_candidates_agg) or None (the generic route).  k-NN retrieval with k beyond the reference rows stays
    generic: its empty slots (-1) have no video."""
    spec = device_aggregation(aggregation)
    if spec is None:
        return None
    if global_k >= 0:
        return "max" if spec[0] == _lib.AGG_MAX else ("agg",) + spec
    return ("agg",) + spec if -global_k <= ntotal else None


class CandidateList(Sequence):
    """Score-descending list of CandidatePair backed by three arrays.

    Behaves like the `List[CandidatePair]` the reference returns (len, indexing, slicing,
    iteration, ==, +); CandidatePair objects are created only for the elements touched.
    """

    def __init__(self, q_ord, r_ord, scores, q_ids, r_ids):
        self.q_ord, self.r_ord, self.scores = q_ord, r_ord, scores
        self._q_ids, self._r_ids = q_ids, r_ids

    def __len__(self):
        return len(self.scores)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return CandidateList(self.q_ord[k], self.r_ord[k], self.scores[k], self._q_ids, self._r_ids)
        return CandidatePair(
            query_id=self._q_ids[self.q_ord[k]], ref_id=self._r_ids[self.r_ord[k]], score=self.scores[k]
        )

    def __eq__(self, other):
        if isinstance(other, (list, tuple, Sequence)):
            return len(self) == len(other) and all(a == b for a, b in zip(self, other))
        return NotImplemented

    def __add__(self, other):
        return list(self) + list(other)

    def __repr__(self):
        head = ", ".join(repr(c) for c in self[:3])
        return f"CandidateList(n={len(self)}, [{head}{', ...' if len(self) > 3 else ''}])"

    def columns(self):
        """(query ids, ref ids, scores) without materialising CandidatePair objects."""
        return ([self._q_ids[q] for q in self.q_ord], [self._r_ids[r] for r in self.r_ord], self.scores)


class CandidateGeneration:
    """vsc/candidates.py:29-40"""

    def __init__(self, references: List[VideoFeature], aggregation: ScoreAggregation):
        self.aggregation = aggregation
        dim = references[0].dimensions()
        self.index = VideoIndex(dim)
        self.index.add(references)

    def query(self, queries: List[VideoFeature], global_k: int) -> List[CandidatePair]:
        route = device_route(self.aggregation, global_k, self.index.index.ntotal)
        if route == "max":
            return self._query_max(queries, global_k)
        if route is not None:
            if global_k < 0:
                logging.warning(KNN_WARNING)
            return self._query_agg(queries, global_k, route[1], route[2])
        matches = self.index.search(queries, global_k=global_k)
        candidates = [self.aggregation.score(match) for match in matches]
        candidates = sorted(candidates, key=lambda match: match.score, reverse=True)
        return candidates

    def _query_max(self, queries: List[VideoFeature], global_k: int) -> CandidateList:
        """One call into libvscmi: search + regroup + max + sort, the hit list never leaves HBM."""
        layout = VideoLayout(queries)
        feats = VideoLayout.features(queries)
        q_ids, r_ids = layout.video_ids, self.index._video_ids
        nq, nr = feats.shape[0], self.index.index.ntotal
        empty = np.zeros(0, dtype=np.int32)
        if nq == 0 or nr == 0 or global_k == 0:
            return CandidateList(empty, empty, np.zeros(0, dtype=np.float32), q_ids, r_ids)
        if feats.shape[1] != self.index.dim:
            raise ValueError(f"expected [n, {self.index.dim}] features, got {feats.shape}")
        row2q = np.ascontiguousarray(layout.row2vid, dtype=np.int32)
        row2r = np.ascontiguousarray(self.index._row2vid, dtype=np.int32)
        cap = int(max(1, min(int(global_k), nq * nr)))
        oq = np.empty(cap, dtype=np.int32)
        orr = np.empty(cap, dtype=np.int32)
        os_ = np.empty(cap, dtype=np.float32)
        n_pairs, n_hits = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.lib().vsc_index_candidates(
            self.index.index.handle, feats.ctypes.data, nq, _lib.MEM_HOST, int(global_k), row2q.ctypes.data,
            row2r.ctypes.data, oq.ctypes.data, orr.ctypes.data, os_.ctypes.data, cap, ctypes.byref(n_pairs),
            ctypes.byref(n_hits)))
        m = n_pairs.value
        return CandidateList(oq[:m].copy(), orr[:m].copy(), os_[:m].copy(), q_ids, r_ids)

    def _query_agg(self, queries: List[VideoFeature], global_k: int, agg: int, top_m: int) -> CandidateList:
        """The same for the other aggregations and for k-NN retrieval (global_k = -k): search or k-NN + regroup +
        aggregate + sort in one call, the hit list never leaves HBM."""
        layout = VideoLayout(queries)
        feats = VideoLayout.features(queries)
        q_ids, r_ids = layout.video_ids, self.index._video_ids
        nq, nr = feats.shape[0], self.index.index.ntotal
        empty = np.zeros(0, dtype=np.int32)
        if nq == 0 or nr == 0 or global_k == 0:
            return CandidateList(empty, empty, np.zeros(0, dtype=np.float32), q_ids, r_ids)
        if feats.shape[1] != self.index.dim:
            raise ValueError(f"expected [n, {self.index.dim}] features, got {feats.shape}")
        row2q = np.ascontiguousarray(layout.row2vid, dtype=np.int32)
        row2r = np.ascontiguousarray(self.index._row2vid, dtype=np.int32)
        n_hits_max = nq * -int(global_k) if global_k < 0 else min(int(global_k), nq * nr)
        cap = int(max(1, min(n_hits_max, len(q_ids) * max(len(r_ids), 1))))
        oq = np.empty(cap, dtype=np.int32)
        orr = np.empty(cap, dtype=np.int32)
        os_ = np.empty(cap, dtype=np.float32)
        n_pairs, n_hits = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.lib().vsc_index_candidates_agg(
            self.index.index.handle, feats.ctypes.data, nq, _lib.MEM_HOST, int(global_k), row2q.ctypes.data,
            row2r.ctypes.data, int(agg), int(top_m), oq.ctypes.data, orr.ctypes.data, os_.ctypes.data, cap,
            ctypes.byref(n_pairs), ctypes.byref(n_hits)))
        m = n_pairs.value
        return CandidateList(oq[:m].copy(), orr[:m].copy(), os_[:m].copy(), q_ids, r_ids)
