"""Temporal localisation of candidate pairs on the MI355X engine.

Class surface of the reference module (`Localization`, `LocalizationWithMetadata`,
`VCSLLocalization`, `VCSLLocalizationMaxSim`, `VCSLLocalizationCandidateScore`, with their
`localize` / `localize_all` / `similarity` / `score` methods;
/root/reference/vsc/baseline/localization.py:16-96).

How it runs here: the constructor uploads both descriptor sets once into a libvscmi TN context
(HBM resident).  A batch then takes one route, the same for `localize_all` and `localize_table` (`_answer`):
`_device_route` picks the launch function of the instance -- the fused Temporal-Network kernel, the DTW / DP one
(`on_device=True`), a subclass's own -- or none; the candidate ids become ordinals once; the launch sends only that
(query ordinal, reference ordinal) list and fills one `BoxTable` (one workgroup per pair computes the frame x frame
similarity on the matrix cores, aligns and scores the boxes); the pairs the kernel did not finish (`status != 0`) --
every pair, when a subclass overrides `score` or `similarity` in a way no kernel can know -- take the reference's
route (`_reference_rows`: similarity matrices on the host, `self.model.forward_sim(...)`, `self.score(...)` per box)
and are spliced back in candidate order.

The two methods differ in the last step only.  `localize_all` converts box corners to timestamps on the host, box by
box (`box_matches`).  `localize_table` returns the same rows as a `vsc.metrics.MatchTable`: the timestamp tables are
uploaded with the descriptors, and the box -> timestamp conversion is device work too (libvscmi vsc_tn_match_rows).
"""
import abc
import ctypes
from typing import Dict, Iterable, Iterator, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from vsc2022_amd import _lib
from vsc2022_amd.vsc.index import VideoFeature, VideoLayout
from vsc2022_amd.vsc.metrics import CandidatePair, Match, MatchTable, _column


class Localization(abc.ABC):
    @abc.abstractmethod
    def localize(self, candidate: CandidatePair) -> List[Match]:
        ...

    def localize_all(self, candidates: List[CandidatePair]) -> List[Match]:
        out: List[Match] = []
        for candidate in candidates:
            out += self.localize(candidate)
        return out


def _timestamp_rows(videos: Sequence[VideoFeature]) -> np.ndarray:
    """float64 [rows, 2] = (start, end) of every frame of the videos, in order; 1-D timestamps become (t, t) rows, as
    `get_timestamps` returns them.  float32, float64 and integers up to 32 bits are exact in float64."""
    parts = []
    for v in videos:
        t = np.asarray(v.timestamps)
        if t.dtype.kind not in "fiu":
            raise TypeError(f"video {v.video_id!r}: timestamps of dtype {t.dtype} cannot be kept on the device")
        parts.append(np.stack([t, t], axis=1) if t.ndim == 1 else t[:, :2])
    if not parts:
        return np.zeros((0, 2), dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([p.astype(np.float64) for p in parts], axis=0))


def _time_dtype(videos: Sequence[VideoFeature], used: np.ndarray) -> np.dtype:
    """dtype of a time column: that of the `timestamps` arrays of the videos that have rows (of all videos when none has),
    their common dtype when they disagree (float32 with float64: float64) -- what a list of their scalars becomes."""
    pool = [videos[k] for k in used] if len(used) else list(videos)
    kinds = {np.asarray(v.timestamps).dtype for v in pool}
    return np.result_type(*kinds) if kinds else np.dtype(np.float64)


class BoxTable(NamedTuple):
    """The device's answer for a batch of n candidate pairs: host arrays, allocated here and filled by a launch function."""

    pair_q: np.ndarray   # int32 [n]: the pairs' query video ordinals ...
    pair_r: np.ndarray   # ... and reference video ordinals
    n_boxes: np.ndarray  # int32 [n]
    boxes: np.ndarray    # int32 [n, TN_MAX_BOXES, 4]: q_lo, r_lo, q_hi, r_hi (frame indices, inclusive ends)
    box_max: np.ndarray  # fp32 [n, TN_MAX_BOXES]: the kernel's MaxSim score of every box
    status: np.ndarray   # int32 [n]: != 0 where the kernel left the pair to the caller; all zero on routes that always finish

    @classmethod
    def zeros(cls, pair_q: np.ndarray, pair_r: np.ndarray) -> "BoxTable":
        n = len(pair_q)
        return cls(pair_q, pair_r, np.zeros(n, dtype=np.int32), np.zeros((n, _lib.TN_MAX_BOXES, 4), dtype=np.int32),
                   np.zeros((n, _lib.TN_MAX_BOXES), dtype=np.float32), np.zeros(n, dtype=np.int32))

    def unfinished(self) -> List[int]:
        return np.flatnonzero(self.status).tolist()


def box_matches(candidates: Sequence[CandidatePair], n_boxes, boxes, box_max, to_match, score,
                spliced: Optional[Mapping[int, List[Match]]] = None) -> List[Match]:
    """A box table as the matches of its batch, pair by pair in candidate order: `to_match(candidate, box)` with the
    score `score(candidate, box_max[k, b])`.  spliced: {pair index: the matches another route found for that pair}; they
    take the pair's place, whatever the table holds for it."""
    spliced = spliced or {}
    matches: List[Match] = []
    for k, candidate in enumerate(candidates):
        if k in spliced:
            matches += spliced[k]
            continue
        for b in range(int(n_boxes[k])):
            match = to_match(candidate, [int(v) for v in boxes[k, b]])
            matches.append(match._replace(score=score(candidate, box_max[k, b])))
    return matches


def rows_table(rows: Iterable[Tuple[int, Match, Tuple[int, int, int, int]]]) -> MatchTable:
    """`(pair index, match, box)` rows (`VCSLLocalization._reference_rows`) collected as columns."""
    rows = list(rows)
    return MatchTable.from_matches([match for _, match, _ in rows], pair=[k for k, _, _ in rows], boxes=[box for _, _, box in rows])


def splice_rows(table: MatchTable, rows) -> MatchTable:
    """The device's rows of a batch with the `(pair index, match, box)` rows of the pairs it did not finish (for which it
    holds none) put in at their pairs' places: candidate order."""
    rest = rows_table(rows)
    if not len(rest):
        return table
    both = MatchTable.concat([table, rest])
    return both.take(np.argsort(both.pair, kind="stable"))


class LocalizationWithMetadata(Localization):
    """Keeps the descriptors of both sides (by video id) -- here: resident in HBM."""

    def __init__(self, queries: List[VideoFeature], refs: List[VideoFeature], device=None, ref_codec: str = "Flat"):
        """ref_codec: how the context stores the reference descriptors ("Flat" / "SQfp16", as vsc.index.VideoIndex).
        "SQfp16" keeps them once, as half floats: every result is that of the same class on the references rounded to
        float16 and converted back.  References whose `feature` arrays are all float16 are handed over as half rows."""
        self._ref_codec_id = _lib.codec_id(ref_codec)  # NotImplementedError for every other string, device or not
        self.ref_codec = ref_codec
        # id -> VideoFeature; a repeated id keeps its last occurrence, as a dict does in the reference
        self.queries: Dict[object, VideoFeature] = {v.video_id: v for v in queries}
        self.refs: Dict[object, VideoFeature] = {v.video_id: v for v in refs}
        self._q_videos, self._r_videos = list(self.queries.values()), list(self.refs.values())
        self._q_ordinal = {v.video_id: n for n, v in enumerate(self._q_videos)}
        self._r_ordinal = {v.video_id: n for n, v in enumerate(self._r_videos)}
        self.device = _lib.default_device() if device is None else int(device)
        self._ctx = ctypes.c_void_p()
        self._upload()

    def _upload(self):
        q_layout, r_layout = VideoLayout(self._q_videos), VideoLayout(self._r_videos)
        q_rows = VideoLayout.features(self._q_videos)
        r_half = len(self._r_videos) > 0 and all(np.asarray(v.feature).dtype == np.float16 for v in self._r_videos)
        if r_half:  # (the rows go down as they are: 2 bytes per element on the host, in staging and in an SQfp16 store)
            r_rows = np.ascontiguousarray(np.concatenate([np.asarray(v.feature) for v in self._r_videos], axis=0))
        else:
            r_rows = VideoLayout.features(self._r_videos)
        if q_rows.size and r_rows.size and q_rows.shape[1] != r_rows.shape[1]:
            raise ValueError("query and reference descriptors differ in dimension")
        dim = q_rows.shape[1] if q_rows.size else (r_rows.shape[1] if r_rows.size else 1)
        _lib.check(_lib.lib().vsc_tn_create_codec(
            q_rows.ctypes.data if q_rows.size else None, q_layout.offsets.ctypes.data, len(self._q_videos),
            r_rows.ctypes.data if r_rows.size else None, int(r_half), r_layout.offsets.ctypes.data, len(self._r_videos),
            int(dim), _lib.MEM_HOST, _lib.MEM_HOST, self._ref_codec_id, self.device, ctypes.byref(self._ctx)))
        # the per-frame [start, end] tables go down with the descriptors (include/vscmi.h, match rows).  Timestamps the
        # device table cannot hold (not numeric) leave `localize_all` as it was; `localize_table` then says why it cannot run
        self._ts_error = None
        try:
            q_ts, r_ts = _timestamp_rows(self._q_videos), _timestamp_rows(self._r_videos)
        except (TypeError, ValueError) as exc:
            self._ts_error = exc
            return
        _lib.check(_lib.lib().vsc_tn_set_timestamps(self._ctx, q_ts.ctypes.data, r_ts.ctypes.data, _lib.MEM_HOST))

    @property
    def ref_bytes(self) -> int:
        """Bytes of HBM the context holds for the reference descriptor rows."""
        return int(_lib.lib().vsc_tn_ref_bytes(self._ctx))

    def __del__(self):
        ctx = getattr(self, "_ctx", None)
        if ctx is not None and ctx.value:
            try:
                _lib.lib().vsc_tn_destroy(ctx)
            except Exception:  # interpreter shutdown
                pass
            self._ctx = None

    def _device_similarity(self, candidate: CandidatePair, bias: float) -> np.ndarray:
        q, r = self._q_ordinal[candidate.query_id], self._r_ordinal[candidate.ref_id]
        out = np.empty((len(self._q_videos[q]), len(self._r_videos[r])), dtype=np.float32)
        _lib.check(_lib.lib().vsc_tn_similarity(self._ctx, q, r, float(bias), out.ctypes.data, out.size, None, None))
        return out

    def similarity(self, candidate: CandidatePair):
        """Frame x frame inner products of the pair (fp32, computed on the GPU)."""
        return self._device_similarity(candidate, 0.0)


class VCSLLocalization(LocalizationWithMetadata):
    """Alignment with a VCSL model: "TN" (GPU; the only one the reference ever asks for), "DTW" / "DP" (host, or GPU with
    `on_device=True`), "HV" (host) -- vcsl.vta.build_vta_model."""

    def __init__(self, queries, refs, model_type, similarity_bias=0.0, device=None, ref_codec="Flat", **kwargs):
        super().__init__(queries, refs, device=device, ref_codec=ref_codec)
        from vsc2022_amd.vcsl.vta import build_vta_model  # late import, as in the reference

        self.model = build_vta_model(model_type, **kwargs)
        self.similarity_bias = similarity_bias

    def similarity(self, candidate: CandidatePair):
        """Similarity plus the optional bias (some aligners dislike negative values)."""
        return self._device_similarity(candidate, self.similarity_bias)

    # -- which route, and the launch functions of the device routes ---------------------------------
    def _device_route(self):
        """The launch function of the device route this instance takes, `launch(candidates, table)` filling a zeroed
        `BoxTable` -- `_launch_tn` for the TN model, `_launch_align` for an on-device DTW / DP model (`on_device=True`) --
        or None for the reference's route: any other model, and a `score` or `similarity` that no kernel can know."""
        from vsc2022_amd.vcsl import aligners
        from vsc2022_amd.vcsl.vta import TN

        stock_scores = (VCSLLocalization.score, VCSLLocalizationMaxSim.score, VCSLLocalizationCandidateScore.score)
        if type(self).score not in stock_scores or type(self).similarity is not VCSLLocalization.similarity:
            return None
        if type(self.model) is TN:
            return self._launch_tn
        if type(self.model) in (aligners.DTW, aligners.DP) and self.model.on_device:
            return self._launch_align
        return None

    def _can_fuse(self) -> bool:
        return self._device_route() == self._launch_tn

    def _can_fuse_align(self) -> bool:
        return self._device_route() == self._launch_align

    def _pair_ordinals(self, candidates):
        n = len(candidates)
        return (np.fromiter((self._q_ordinal[c.query_id] for c in candidates), dtype=np.int32, count=n),
                np.fromiter((self._r_ordinal[c.ref_id] for c in candidates), dtype=np.int32, count=n))

    def _launch_tn(self, candidates, table: BoxTable):
        """The fused Temporal-Network kernel (libvscmi vsc_tn_localize); finishes every pair."""
        _lib.check(_lib.lib().vsc_tn_localize(
            self._ctx, table.pair_q.ctypes.data, table.pair_r.ctypes.data, len(table.pair_q), _lib.MEM_HOST,
            ctypes.byref(self.model.params), float(self.similarity_bias), table.n_boxes.ctypes.data, table.boxes.ctypes.data,
            table.box_max.ctypes.data, _lib.MEM_HOST))

    def _launch_align(self, candidates, table: BoxTable):
        """The DTW / DP kernels (libvscmi vsc_tn_align); `status` names the pairs they hand back (too long for their LDS
        state, too many boxes)."""
        _lib.check(_lib.lib().vsc_tn_align(
            self._ctx, table.pair_q.ctypes.data, table.pair_r.ctypes.data, len(table.pair_q), _lib.MEM_HOST,
            ctypes.byref(self.model.params), float(self.similarity_bias), table.n_boxes.ctypes.data, table.boxes.ctypes.data,
            table.box_max.ctypes.data, table.status.ctypes.data, _lib.MEM_HOST))

    def _aligned_boxes(self, candidates: Sequence[CandidatePair]):
        """`(n_boxes, boxes, box_max, status)` of one `_launch_align`."""
        table = BoxTable.zeros(*self._pair_ordinals(candidates))
        self._launch_align(candidates, table)
        return table.n_boxes, table.boxes, table.box_max, table.status

    def _to_match(self, candidate: CandidatePair, box) -> Match:
        """Box corners are frame indices with inclusive ends: the segment runs from the start of the
        first frame to the end of the last one."""
        x1, y1, x2, y2 = box
        query, ref = self.queries[candidate.query_id], self.refs[candidate.ref_id]
        return Match(query_id=candidate.query_id, ref_id=candidate.ref_id, score=0.0,
                     query_start=query.get_timestamps(x1)[0], query_end=query.get_timestamps(x2)[1],
                     ref_start=ref.get_timestamps(y1)[0], ref_end=ref.get_timestamps(y2)[1])

    def _reference_rows(self, candidates: Sequence[CandidatePair], pair_index: Sequence[int]) -> Iterator[Tuple[int, Match, tuple]]:
        """The reference's route: matrices on the host, any model, any score hook.  Yields `(pair index, match, box)` in
        candidate order (pair_index: the candidates' positions in the batch).  A generator: no matrix is asked for before
        the first row is, and none at all for no candidates."""
        named = [(f"{c.query_id}-{c.ref_id}", self.similarity(c)) for c in candidates]
        if not named:
            return
        results = self.model.forward_sim(named)
        assert len(results) == len(named)
        for k, candidate, (key, sim), (name, pair_boxes) in zip(pair_index, candidates, named, results):
            assert key == name
            for box in pair_boxes:
                box = tuple(int(v) for v in box)
                match = self._to_match(candidate, box)
                yield k, match._replace(score=self.score(candidate, match, box, sim)), box

    def _answer(self, candidates):
        """The one route of a non-empty batch: `(table, rest)`.  table: the `BoxTable` the device route filled, None
        without one; rest: the reference route's rows (`_reference_rows`, not started) of the pairs the device did not
        finish -- of all pairs without a device route."""
        launch = self._device_route()
        if launch is None:
            return None, self._reference_rows(candidates, range(len(candidates)))
        table = BoxTable.zeros(*self._pair_ordinals(candidates))
        launch(candidates, table)
        left = table.unfinished()
        return table, self._reference_rows([candidates[k] for k in left], left)

    def localize_all(self, candidates: List[CandidatePair]) -> List[Match]:
        candidates = list(candidates)
        if not candidates:
            return []
        table, rest = self._answer(candidates)
        if table is None:
            return [match for _, match, _ in rest]
        spliced = {k: [] for k in table.unfinished()}
        for k, match, _ in rest:
            spliced[k].append(match)
        return box_matches(candidates, table.n_boxes, table.boxes, table.box_max, self._to_match, self._fused_score, spliced)

    def localize(self, candidate: CandidatePair) -> List[Match]:
        return self.localize_all([candidate])

    def localize_table(self, candidates: List[CandidatePair]) -> MatchTable:
        """`localize_all(candidates)` as a MatchTable: the same rows in the same order, values and dtypes included
        (`localize_table(c).to_matches() == localize_all(c)`, and `write_csv` writes the same file).  On the device
        routes the timestamps are gathered on the device and there is no per-box Python."""
        candidates = candidates if hasattr(candidates, "columns") else list(candidates)
        if len(candidates) == 0:
            return MatchTable.empty()
        table, rest = self._answer(candidates)
        if table is None:
            return rows_table(rest)
        return splice_rows(self._device_rows(candidates, table), rest)  # (the device's rows first, then the matrices of `rest`)

    def _device_rows(self, candidates, table: BoxTable) -> MatchTable:
        """The box table of a batch -> its match rows, by the engine's match-rows stage (vsc_tn_match_rows: row offsets,
        timestamp gathers and the dense table are device work); ids and column dtypes are attached here."""
        if self._ts_error is not None:
            raise ValueError(f"localize_table needs numeric timestamps: {self._ts_error}")
        pair_q, pair_r, n_boxes, boxes, box_max, _ = table
        cap = int(n_boxes.sum(dtype=np.int64))
        pair = np.empty(cap, dtype=np.int32)
        corners = np.empty((cap, 4), dtype=np.int32)
        score = np.empty(cap, dtype=np.float32)
        times = np.empty((cap, 4), dtype=np.float64)
        n_rows = ctypes.c_int64(0)
        _lib.check(_lib.lib().vsc_tn_match_rows(
            self._ctx, pair_q.ctypes.data, pair_r.ctypes.data, len(pair_q), _lib.MEM_HOST, n_boxes.ctypes.data,
            boxes.ctypes.data, box_max.ctypes.data, _lib.MEM_HOST, pair.ctypes.data, corners.ctypes.data, score.ctypes.data,
            times.ctypes.data, cap, _lib.MEM_HOST, ctypes.byref(n_rows)))
        assert n_rows.value == cap
        q_ord, r_ord = pair_q[pair], pair_r[pair]
        q_t = _time_dtype(self._q_videos, np.unique(q_ord))
        r_t = _time_dtype(self._r_videos, np.unique(r_ord))
        q_ids = MatchTable._ids(v.video_id for v in self._q_videos)
        r_ids = MatchTable._ids(v.video_id for v in self._r_videos)
        return MatchTable(q_ids[q_ord], r_ids[r_ord], self._fused_score_column(candidates, pair, score),
                          times[:, 0].astype(q_t), times[:, 1].astype(q_t), times[:, 2].astype(r_t),
                          times[:, 3].astype(r_t), pair.astype(np.int64), corners)

    def score(self, candidate: CandidatePair, match: Match, box, similarity) -> float:
        return 1.0

    def _fused_score(self, candidate: CandidatePair, box_max) -> float:
        return 1.0

    def _fused_score_column(self, candidates, pair: np.ndarray, box_max: np.ndarray) -> np.ndarray:
        """`_fused_score` of every row at once."""
        return np.ones(len(pair), dtype=np.float64)


class VCSLLocalizationMaxSim(VCSLLocalization):
    """Box score = best frame similarity inside the box (half-open slice: the last row and column of
    the box are left out, exactly like the reference's `similarity[x1:x2, y1:y2]`), bias removed."""

    def score(self, candidate: CandidatePair, match: Match, box, similarity) -> float:
        x1, y1, x2, y2 = box
        return similarity[x1:x2, y1:y2].max() - self.similarity_bias

    def _fused_score(self, candidate: CandidatePair, box_max) -> float:
        return box_max  # computed by the kernel as max(sims[x1:x2, y1:y2]) - bias

    def _fused_score_column(self, candidates, pair, box_max):
        return box_max


class VCSLLocalizationCandidateScore(VCSLLocalization):
    """Box score = the retrieval score of the candidate pair."""

    def score(self, candidate: CandidatePair, match: Match, box, similarity) -> float:
        return candidate.score

    def _fused_score(self, candidate: CandidatePair, box_max) -> float:
        return candidate.score

    def _fused_score_column(self, candidates, pair, box_max):
        # (the scores keep the type they have in the candidates: float32 from the engine's lists, float64 from Python floats)
        columns = getattr(candidates, "columns", None)
        scores = np.asarray(columns()[2]) if columns is not None else _column([c.score for c in candidates])
        return scores[pair]
