"""Records, CSV formats and the two challenge metrics (candidate micro-AP, segment-level AP).

Public names and semantics follow the reference's `vsc/metrics.py` (cited per symbol; paths relative
to /root/reference) so that files and scores are interchangeable; the implementation is array-first
(10^5..10^6 predictions must not spend minutes in per-object Python).  Values are pinned against the
reference by fixture `tests/golden/g7_metrics.npz`.
"""
import bisect
import dataclasses
import enum
import math
from typing import Collection, Dict, Iterable, List, NamedTuple, Optional, TextIO, Tuple, Union

import numpy as np


class Dataset(enum.Enum):
    """Which side of the challenge a video id belongs to; the value is the id prefix (metrics.py:21-23)."""

    QUERIES = "Q"
    REFS = "R"


def format_video_id(video_id: Union[str, int], dataset: Optional[Dataset]) -> str:
    """Canonical string id: integers become `<prefix>%06d`, strings are checked against the prefix
    (metrics.py:26-40)."""
    if isinstance(video_id, (int, np.integer)):
        if dataset is None:
            raise ValueError("Unable to convert integer video_id without a Dataset enum")
        return "%s%06d" % (dataset.value, int(video_id))
    if not isinstance(video_id, str):
        raise AssertionError(f"unexpected video_id: {video_id} of type {type(video_id)}")
    if dataset is not None and not video_id.startswith(dataset.value):
        raise AssertionError(f"dataset mismatch? got {video_id} for dataset {dataset}")
    return video_id


def _pandas():
    import pandas  # deferred: `import vsc2022_amd` stays light

    return pandas


def _pair_columns(pairs) -> Tuple[list, list, np.ndarray]:
    """(query ids, ref ids, scores) of a collection of CandidatePair (array-backed lists expose
    `columns()` and are never expanded into objects)."""
    columns = getattr(pairs, "columns", None)
    if columns is not None:
        q, r, s = columns()
        return list(q), list(r), np.asarray(s, dtype=np.float64)
    pairs = list(pairs)
    return ([p.query_id for p in pairs], [p.ref_id for p in pairs],
            np.fromiter((p.score for p in pairs), dtype=np.float64, count=len(pairs)))


@dataclasses.dataclass
class CandidatePair:
    """A (query video, reference video) pair with a confidence (metrics.py:43-93)."""

    query_id: str
    ref_id: str
    score: float

    @classmethod
    def to_dataframe(cls, candidates: Collection["CandidatePair"]):
        q, r, _ = _pair_columns(candidates)
        if not q:  # the reference builds a column-less frame from an empty list
            return _pandas().DataFrame([])
        # scores keep their own dtype (fp32 from the engine) so that the CSV text matches the reference's
        raw_scores = candidates.columns()[2] if hasattr(candidates, "columns") else [c.score for c in candidates]
        return _pandas().DataFrame({
            "query_id": [format_video_id(x, Dataset.QUERIES) for x in q],
            "ref_id": [format_video_id(x, Dataset.REFS) for x in r],
            "score": raw_scores,
        })

    @classmethod
    def write_csv(cls, candidates: Collection["CandidatePair"], file: Union[str, TextIO]):
        cls.to_dataframe(candidates).to_csv(file, index=False)

    @classmethod
    def read_csv(cls, file: Union[str, TextIO]) -> List["CandidatePair"]:
        table = _pandas().read_csv(file)
        rows = zip(table["query_id"], table["ref_id"], table["score"])
        return [cls(format_video_id(q, Dataset.QUERIES), format_video_id(r, Dataset.REFS), s) for q, r, s in rows]

    @classmethod
    def from_matches(cls, matches: Collection["Match"]) -> List["CandidatePair"]:
        """One pair per (query, ref) with the best segment score, floored at 0 as the reference's
        defaultdict(float) does (metrics.py:84-93)."""
        best: Dict[Tuple[str, str], float] = {}
        for m in matches:
            key = (m.query_id, m.ref_id)
            best[key] = max(m.score, best.get(key, 0.0))
        return [cls(q, r, s) for (q, r), s in best.items()]


@dataclasses.dataclass
class PrecisionRecallCurve:
    """metrics.py:96-111"""

    precisions: np.ndarray
    recalls: np.ndarray
    scores: np.ndarray

    def plot(self, ax=None, **kwargs):
        if ax is None:
            import matplotlib.pyplot as plt

            ax = plt.subplots()[1]
            ax.set(xlabel="recall", ylabel="precision", xlim=(0, 1.05), ylim=(0, 1.05))
        ax.plot(self.recalls, self.precisions, **kwargs)
        return ax


@dataclasses.dataclass
class AveragePrecision:
    """metrics.py:114-118"""

    ap: float
    pr_curve: PrecisionRecallCurve
    simple_ap: Optional[float] = None


# ------------------------------------------------------------------------------------ intervals

def _coalesce(intervals: Iterable[Tuple[float, float]]) -> List[Tuple[float, float]]:
    """Union of closed intervals as a sorted list of disjoint ones (touching intervals merge)."""
    merged: List[Tuple[float, float]] = []
    for lo, hi in sorted(intervals):
        if merged and lo <= merged[-1][1]:
            if hi > merged[-1][1]:
                merged[-1] = (merged[-1][0], hi)
        else:
            merged.append((lo, hi))
    return merged


class Intervals:
    """A union of intervals on one time axis (metrics.py:120-174)."""

    intervals: List[Tuple[float, float]]

    def __init__(self, intervals: Optional[List[Tuple[float, float]]] = None):
        self.intervals = _coalesce(intervals or [])

    def add(self, interval: Tuple[float, float]):
        """Insert one interval, keeping the list sorted and disjoint (O(log n + merged))."""
        lo, hi = interval
        items = self.intervals
        k = bisect.bisect_left(items, (lo, hi))
        if k > 0 and items[k - 1][1] >= lo:  # overlaps its left neighbour
            k -= 1
            lo, hi = items[k][0], max(items[k][1], hi)
        end = k
        while end < len(items) and items[end][0] <= hi:
            hi = max(hi, items[end][1])
            end += 1
        items[k:end] = [(lo, hi)]

    def union(self, intervals: "Intervals") -> "Intervals":
        return Intervals(self.intervals + intervals.intervals)

    def total_length(self) -> float:
        total = 0.0
        for lo, hi in self.intervals:
            total += hi - lo
        return total

    def intersect_length(self, intervals: "Intervals") -> float:
        """|A n B| = |A| + |B| - |A u B|."""
        return self.total_length() + intervals.total_length() - self.union(intervals).total_length()

    def __repr__(self):
        return str(self.intervals)

    __str__ = __repr__


class Axis(enum.Enum):
    QUERY = enum.auto()
    REF = enum.auto()


class Match(NamedTuple):
    """A copied segment: ground truth or prediction (metrics.py:182-235)."""

    query_id: str
    ref_id: str
    score: float
    query_start: float
    query_end: float
    ref_start: float
    ref_end: float

    def pair_id(self):
        return (self.query_id, self.ref_id)

    def interval(self, axis: Axis) -> Tuple[float, float]:
        return (self.query_start, self.query_end) if axis == Axis.QUERY else (self.ref_start, self.ref_end)

    def intersection_area(self, bbox: "Match") -> float:
        width = min(self.query_end, bbox.query_end) - max(self.query_start, bbox.query_start)
        height = min(self.ref_end, bbox.ref_end) - max(self.ref_start, bbox.ref_start)
        return abs(max(width, 0) * max(height, 0))

    def overlaps(self, bbox: "Match") -> bool:
        return self.intersection_area(bbox) > 0.0

    @classmethod
    def write_csv(cls, matches: Collection["Match"], file: Union[str, TextIO]):
        _pandas().DataFrame([m._asdict() for m in matches], columns=cls._fields).to_csv(file, index=False)

    @classmethod
    def read_csv(cls, file: Union[str, TextIO], is_gt=False, check=True) -> List["Match"]:
        table = _pandas().read_csv(file)
        table["query_id"] = [format_video_id(x, Dataset.QUERIES) for x in table["query_id"]]
        table["ref_id"] = [format_video_id(x, Dataset.REFS) for x in table["ref_id"]]
        if is_gt:
            table["score"] = 1.0
        if check:
            for field in cls._fields:
                assert not table[field].isna().any()
        return [cls(**row) for row in table.to_dict("records")]


def _id_column(series, dataset: Dataset) -> np.ndarray:
    """`format_video_id` over a CSV column: integers become `<prefix>%06d`, strings are checked against the prefix -- one
    vectorised pass per column; a column that mixes both goes value by value."""
    pd = _pandas()
    out = np.empty(len(series), dtype=object)
    if pd.api.types.is_integer_dtype(series.dtype):
        out[:] = (dataset.value + series.astype(str).str.zfill(6)).to_numpy(dtype=object)
    elif len(series) and series.map(type).eq(str).all():
        if not series.str.startswith(dataset.value).all():
            bad = series[~series.str.startswith(dataset.value)].iloc[0]
            raise AssertionError(f"dataset mismatch? got {bad} for dataset {dataset}")
        out[:] = series.to_numpy(dtype=object)
    else:
        out[:] = [format_video_id(x, dataset) for x in series]
    return out


def _column(values, like: Optional[np.ndarray] = None) -> np.ndarray:
    """A list of scalars as an array of the dtype those scalars carry (np.float32 scalars -> float32, Python floats ->
    float64); an empty list takes the dtype of `like`."""
    values = list(values)
    if not values:
        return np.zeros(0, dtype=like.dtype if like is not None else np.float64)
    return np.asarray(values)


@dataclasses.dataclass
class MatchTable:
    """The rows of a `List[Match]` as columns: what the match-rows stage of the engine returns (include/vscmi.h,
    vsc_tn_match_rows) and what `write_csv` needs.  No per-row Python anywhere but in `to_matches`.

    Every column keeps the dtype the scalar route yields -- scores float32 from the MaxSim kernel, float64 from Python
    floats; times in the dtype of the videos' `timestamps` arrays -- because the CSV text depends on it: `write_csv`
    writes byte for byte what `Match.write_csv(table.to_matches(), file)` writes.

    pair: index of the row's candidate in the candidate list the table came from; boxes: [n, 4] int32 frame indices
    q_lo, r_lo, q_hi, r_hi (inclusive ends)."""

    query_id: np.ndarray
    ref_id: np.ndarray
    score: np.ndarray
    query_start: np.ndarray
    query_end: np.ndarray
    ref_start: np.ndarray
    ref_end: np.ndarray
    pair: np.ndarray
    boxes: np.ndarray

    def __post_init__(self):
        n = len(self.score)
        for field in Match._fields + ("pair", "boxes"):
            assert len(getattr(self, field)) == n, f"column {field} has {len(getattr(self, field))} rows, score has {n}"

    def __len__(self):
        return len(self.score)

    @staticmethod
    def _ids(values) -> np.ndarray:
        values = list(values)
        out = np.empty(len(values), dtype=object)  # (never a numpy string array: ids keep their own type)
        out[:] = values
        return out

    @classmethod
    def empty(cls, score_dtype=np.float64, time_dtype=np.float64) -> "MatchTable":
        t = np.zeros(0, dtype=time_dtype)
        return cls(cls._ids([]), cls._ids([]), np.zeros(0, dtype=score_dtype), t, t.copy(), t.copy(), t.copy(),
                   np.zeros(0, dtype=np.int64), np.zeros((0, 4), dtype=np.int32))

    @classmethod
    def from_matches(cls, matches: Collection[Match], pair=None, boxes=None) -> "MatchTable":
        """Columns of a list of Match (the host routes); pair / boxes default to -1."""
        matches = list(matches)
        n = len(matches)
        return cls(cls._ids(m.query_id for m in matches), cls._ids(m.ref_id for m in matches),
                   _column(m.score for m in matches), _column(m.query_start for m in matches),
                   _column(m.query_end for m in matches), _column(m.ref_start for m in matches),
                   _column(m.ref_end for m in matches),
                   np.full(n, -1, dtype=np.int64) if pair is None else np.asarray(pair, dtype=np.int64).reshape(n),
                   np.full((n, 4), -1, dtype=np.int32) if boxes is None else np.asarray(boxes, dtype=np.int32).reshape(n, 4))

    @classmethod
    def read_csv(cls, file: Union[str, TextIO], is_gt=False, check=True) -> "MatchTable":
        """`from_matches(Match.read_csv(file, is_gt, check))` column for column, without the rows in between: the
        columns come straight from pandas (ids formatted per column, not per row)."""
        table = _pandas().read_csv(file)
        if is_gt:
            table["score"] = 1.0
        if check:
            for field in Match._fields:
                assert not table[field].isna().any()
        n = len(table)
        if n == 0:
            return cls.empty()
        columns = [_id_column(table["query_id"], Dataset.QUERIES), _id_column(table["ref_id"], Dataset.REFS)]
        columns += [table[field].to_numpy() for field in Match._fields[2:]]
        return cls(*columns, np.full(n, -1, dtype=np.int64), np.full((n, 4), -1, dtype=np.int32))

    def to_matches(self) -> List[Match]:
        """The rows as Match tuples; every value is the numpy scalar of its column (as the per-box route yields them)."""
        return [Match(*row) for row in zip(*(getattr(self, field) for field in Match._fields))]

    def to_dataframe(self):
        return _pandas().DataFrame({field: getattr(self, field) for field in Match._fields}, columns=Match._fields)

    def write_csv(self, file: Union[str, TextIO]):
        self.to_dataframe().to_csv(file, index=False)

    def take(self, index) -> "MatchTable":
        """The rows `index` (an index array or a boolean mask), in that order."""
        return MatchTable(*(getattr(self, f.name)[index] for f in dataclasses.fields(self)))

    @classmethod
    def concat(cls, tables: Iterable["MatchTable"], pair_offsets: Optional[Iterable[int]] = None) -> "MatchTable":
        """Tables one after the other.  pair_offsets: added to each table's `pair` column (batches of one candidate
        list).  Empty tables do not vote on a column's dtype, as rows that do not exist cannot in a list of Match."""
        tables = list(tables)
        offsets = [0] * len(tables) if pair_offsets is None else [int(o) for o in pair_offsets]
        assert len(offsets) == len(tables)
        if not tables:
            return cls.empty()
        voting = [(t, o) for t, o in zip(tables, offsets) if len(t)] or [(tables[0], offsets[0])]
        columns = []
        for f in dataclasses.fields(cls):
            parts = [getattr(t, f.name) + o if f.name == "pair" else getattr(t, f.name) for t, o in voting]
            columns.append(parts[0] if len(parts) == 1 else np.concatenate(parts, axis=0))
        return cls(*columns)

    def __add__(self, other: "MatchTable") -> "MatchTable":
        return MatchTable.concat([self, other])


class VideoPair:
    """Running overlap statistics of one (query, ref) pair (metrics.py:238-301).

    A ground-truth segment counts towards the intersection only once some prediction overlaps it in
    area (both axes), as in the reference; the state is incremental -- which ground-truth segments
    are "awake" and the merged prediction intervals are carried from call to call instead of being
    rebuilt from every earlier prediction.
    """

    gts: List[Match]
    preds: List[Match]

    def __init__(self):
        self.gts, self.preds = [], []
        self.intersections = {axis: 0.0 for axis in Axis}
        self.totals = {axis: 0.0 for axis in Axis}
        self._awake: List[bool] = []
        self._covered = {axis: Intervals() for axis in Axis}

    def total_gt_length(self, axis: Axis) -> float:
        return Intervals([g.interval(axis) for g in self.gts]).total_length()

    def total_pred_length(self, axis: Axis) -> float:
        return Intervals([p.interval(axis) for p in self.preds]).total_length()

    def gt_overlaps(self, gt: Match) -> bool:
        return any(gt.overlaps(p) for p in self.preds)

    def add_gt(self, bbox: Match):
        self.gts.append(bbox)
        self._awake.append(self.gt_overlaps(bbox))

    def add_prediction(self, bbox: Match) -> Tuple[Dict[Axis, float], Dict[Axis, float]]:
        """Returns the change of (intersection with ground truth, covered length) per axis."""
        self.preds.append(bbox)
        for k, gt in enumerate(self.gts):
            if not self._awake[k] and gt.overlaps(bbox):
                self._awake[k] = True
        d_inter, d_total = {}, {}
        for axis in Axis:
            covered = self._covered[axis]
            covered.add(bbox.interval(axis))
            truth = Intervals([g.interval(axis) for g, on in zip(self.gts, self._awake) if on])
            inter, total = covered.intersect_length(truth), covered.total_length()
            d_inter[axis], d_total[axis] = inter - self.intersections[axis], total - self.totals[axis]
            self.intersections[axis], self.totals[axis] = inter, total
        return d_inter, d_total


def match_metric(gts: Collection[Match], predictions: Collection[Match]) -> AveragePrecision:
    """Segment-level AP of the matching track (metrics.py:304-378): AP = sum_i P(i) * dR(i) with
    P = sqrt(P_query * P_ref) and R = sqrt(R_query * R_ref); predictions with equal scores enter as
    one group before the curve is sampled."""
    ranked = sorted(predictions, key=lambda m: m.score, reverse=True)
    per_pair: Dict[Tuple[str, str], VideoPair] = {}
    for gt in gts:
        per_pair.setdefault(gt.pair_id(), VideoPair()).add_gt(gt)
    # per-axis ground-truth length, accumulated pair by pair (the reference's summation order)
    truth_length = {axis: 0.0 for axis in Axis}
    for pair in per_pair.values():
        for axis in Axis:
            truth_length[axis] += pair.total_gt_length(axis)

    inter = {axis: 0.0 for axis in Axis}
    covered = {axis: 0.0 for axis in Axis}
    ap, recall = 0.0, 0.0
    points = []  # (recall, precision, score)
    cursor = 0
    while cursor < len(ranked):
        score = ranked[cursor].score
        while cursor < len(ranked) and ranked[cursor].score == score:
            pred = ranked[cursor]
            d_inter, d_total = per_pair.setdefault(pred.pair_id(), VideoPair()).add_prediction(pred)
            for axis in Axis:
                inter[axis] += d_inter[axis]
                covered[axis] += d_total[axis]
            cursor += 1
        r_now = math.sqrt((inter[Axis.QUERY] / truth_length[Axis.QUERY]) * (inter[Axis.REF] / truth_length[Axis.REF]))
        p_now = math.sqrt((inter[Axis.QUERY] / covered[Axis.QUERY]) * (inter[Axis.REF] / covered[Axis.REF]))
        gain = r_now - recall
        ap += p_now * gain
        recall = r_now
        if gain > 0:
            points.append((recall, p_now, score))
    curve = PrecisionRecallCurve(np.array([p[1] for p in points]), np.array([p[0] for p in points]),
                                 np.array([p[2] for p in points]))
    return AveragePrecision(ap, curve)


@dataclasses.dataclass
class MatchingTrackMetrics:
    """metrics.py:381-386"""

    segment_ap: AveragePrecision      # the matching-track metric
    pairwise_micro_ap: AveragePrecision  # pair retrieval only, no localisation


def pair_ordinals(gt: MatchTable, pred: MatchTable) -> Tuple[np.ndarray, np.ndarray, int, int]:
    """(ordinal per ground-truth row, ordinal per prediction row, pairs, ground-truth pairs): the (query, ref) pairs of both
    tables numbered in first-appearance order, the ground truth's first -- the order of the host's dict of VideoPair.
    `pandas.factorize` numbers in order of appearance; no per-row Python."""
    pd = _pandas()
    n_gt = len(gt)
    q_code, q_names = pd.factorize(np.concatenate([gt.query_id, pred.query_id]).astype(object))
    r_code, r_names = pd.factorize(np.concatenate([gt.ref_id, pred.ref_id]).astype(object))
    code, names = pd.factorize(q_code.astype(np.int64) * max(len(r_names), 1) + r_code)
    n_gt_pairs = int(code[:n_gt].max()) + 1 if n_gt else 0
    return code[:n_gt].astype(np.int32), code[n_gt:].astype(np.int32), len(names), n_gt_pairs


def _times64(table: MatchTable) -> np.ndarray:
    return np.ascontiguousarray(np.stack([np.asarray(getattr(table, f), dtype=np.float64) for f in Match._fields[3:]], axis=1)
                                .reshape(len(table), 4))


def segment_ap_tail(scores: np.ndarray, sums: np.ndarray, gt_len) -> AveragePrecision:
    """The end of `match_metric`, vectorised over the groups of equal scores: scores [g], sums [g, 4] = the running
    intersection (query, ref) and covered length (query, ref) at each group end, gt_len = the ground truth's length per
    axis (what libvscmi's vsc_match_metric returns).  Every operation is a correctly rounded IEEE one and `np.cumsum` adds
    in order, so the values are the host loop's.  Raises where Python's float arithmetic raises: ZeroDivisionError for a
    divisor of 0.0, ValueError for the square root of a negative product -- whichever the loop meets first."""
    tq, tr = float(gt_len[0]), float(gt_len[1])
    if len(scores) == 0:
        return AveragePrecision(0.0, PrecisionRecallCurve(np.array([]), np.array([]), np.array([])))
    if tq == 0.0 or tr == 0.0:
        raise ZeroDivisionError("float division by zero")
    iq, ir, cq, cr = (np.ascontiguousarray(sums[:, k]) for k in range(4))
    with np.errstate(all="ignore"):
        recall_sq = (iq / tq) * (ir / tr)
        no_cover = (cq == 0.0) | (cr == 0.0)
        precision_sq = (iq / cq) * (ir / cr)
        trouble = np.flatnonzero((recall_sq < 0) | no_cover | (precision_sq < 0))
        if len(trouble):  # the loop stops at its first: sqrt of the recall term, the divisions, sqrt of the precision term
            k = trouble[0]
            if recall_sq[k] < 0 or not no_cover[k]:
                raise ValueError("math domain error")
            raise ZeroDivisionError("float division by zero")
        recall, precision = np.sqrt(recall_sq), np.sqrt(precision_sq)
        gain = np.diff(np.r_[0.0, recall])
        ap = float(np.cumsum(precision * gain)[-1])
    at = gain > 0
    return AveragePrecision(ap, PrecisionRecallCurve(precision[at], recall[at], np.asarray(scores, dtype=np.float64)[at]))


def device_group_sums(gt_pair, gt_times, gt_first, n_gt_pairs, pred_pair, pred_score, pred_times, n_pairs, device=0):
    """libvscmi's vsc_match_metric: (scores [g], sums [g, 4], gt_len [2], stats [8]).  The ground-truth arrays and the
    prediction arrays are numpy arrays (host) or torch tensors in HBM, each side as a whole; gt_first may be None (the
    ground truth's pairs are 0 .. n_gt_pairs - 1)."""
    import ctypes

    from vsc2022_amd import _lib

    def side(arrays):
        if all(isinstance(a, np.ndarray) or a is None for a in arrays):
            arrays = [None if a is None else np.ascontiguousarray(a) for a in arrays]
        pointers = [_lib.ptr(a) for a in arrays]
        kinds = {m for (p, m), a in zip(pointers, arrays) if a is not None}
        assert len(kinds) <= 1, "one side's arrays live in one memory"
        return arrays, [p for p, _ in pointers], (kinds.pop() if kinds else _lib.MEM_HOST)

    n_gt, n_pred = len(gt_pair), len(pred_pair)
    gt_keep, gt_ptr, gt_mem = side([gt_pair, gt_times, gt_first])
    pred_keep, pred_ptr, pred_mem = side([pred_pair, pred_score, pred_times])
    for a, dt in zip(gt_keep + pred_keep, ("int32", "float64", "int32", "int32", "float64", "float64")):
        assert a is None or str(a.dtype).endswith(dt), f"vsc_match_metric wants {dt}, got {a.dtype}"
    L = _lib.lib()
    cap = n_pred
    scores, sums = np.empty(cap, dtype=np.float64), np.empty((cap, 4), dtype=np.float64)
    gt_len, stats, n_groups = np.zeros(2, dtype=np.float64), np.zeros(8, dtype=np.int64), ctypes.c_int64(0)
    _lib.check(L.vsc_match_metric(gt_ptr[0], gt_ptr[1], n_gt, gt_ptr[2], int(n_gt_pairs), gt_mem, pred_ptr[0], pred_ptr[1], pred_ptr[2],
                                  n_pred, pred_mem, int(n_pairs), scores.ctypes.data, sums.ctypes.data, cap, ctypes.byref(n_groups),
                                  gt_len.ctypes.data, stats.ctypes.data, int(device)))
    return scores[:n_groups.value], sums[:n_groups.value], gt_len, stats


def match_metric_table(gt: MatchTable, pred: MatchTable, device: int = 0) -> AveragePrecision:
    """Segment-level AP of two MatchTables on the device (libvscmi's vsc_match_metric; include/vscmi.h).

    Equals `match_metric(gt64.to_matches(), pred64.to_matches())` bit for bit in `ap` and the curve, gt64 / pred64 being
    the tables with score and times cast to float64 (exact).  The table route ALWAYS computes in float64: with float32
    numpy scalars the host walk computes in float32 under numpy's promotion rules, a different function.  Where Python's
    float arithmetic raises on the host -- ZeroDivisionError for a ground truth of length 0.0 on an axis or a covered length
    of 0.0 at a group end, ValueError for the square root of a negative product -- this raises the same type (with numpy
    scalars the host's division only warns and yields nan).  Preconditions of this route only: non-finite scores or times,
    `end < start` on an axis and more than `_lib.METRIC_MAX_PAIR_ROWS` rows in one (query, ref) pair raise ValueError.
    No predictions: AveragePrecision(0.0, empty curve), as the host."""
    if len(pred) == 0:
        return segment_ap_tail(np.zeros(0), np.zeros((0, 4)), np.zeros(2))
    gt_pair, pred_pair, n_pairs, n_gt_pairs = pair_ordinals(gt, pred)
    scores, sums, gt_len, _ = device_group_sums(gt_pair, _times64(gt), None, n_gt_pairs, pred_pair,
                                                np.ascontiguousarray(pred.score, dtype=np.float64), _times64(pred), n_pairs, device)
    return segment_ap_tail(scores, sums, gt_len)


def pairwise_ap_table(gt: MatchTable, pred: MatchTable) -> AveragePrecision:
    """`average_precision(CandidatePair.from_matches(gt), CandidatePair.from_matches(pred))` from two MatchTables, bit for
    bit in `ap`, `simple_ap` and the curve: one pair per (query, ref) in first-appearance order with its best score
    floored at 0.0, then integer counting -- vectorised numpy on the host, no kernel."""
    _, pred_pair, n_pairs, n_gt_pairs = pair_ordinals(gt, pred)
    if len(pred) == 0:
        canonical, scores, hit = 0.0, np.zeros(0, dtype=np.float64), np.zeros(0, dtype=bool)
    else:
        pairs, first = np.unique(pred_pair, return_index=True)
        pairs = pairs[np.argsort(first, kind="stable")]  # the prediction's pairs in first-appearance order
        slot = np.empty(n_pairs, dtype=np.int64)
        slot[pairs] = np.arange(len(pairs))
        scores = np.zeros(len(pairs), dtype=np.float64)
        np.maximum.at(scores, slot[pred_pair], np.asarray(pred.score, dtype=np.float64))
        hit = pairs < n_gt_pairs
        if not np.isfinite(scores).all():
            raise ValueError("Scores must be finite.")
        n_found = int(hit.sum())
        canonical = _threshold_ap(hit.astype(np.float64), scores) * (n_found / n_gt_pairs) if n_found else 0.0
    order = np.argsort(-scores, kind="stable")
    hit = hit[order]
    found = np.cumsum(hit)
    precision = found / (np.arange(len(hit)) + 1)
    recall = found / n_gt_pairs
    simple_ap = np.sum(precision * hit) / n_gt_pairs
    at = np.flatnonzero(hit)
    return AveragePrecision(ap=canonical, pr_curve=PrecisionRecallCurve(precision[at], recall[at], scores[order][at]),
                            simple_ap=simple_ap)


def evaluate_matching_track(ground_truth_filename: str, predictions_filename: str, on_device: bool = False
                            ) -> MatchingTrackMetrics:
    """Both metrics from two CSV files with the `Match` columns in any order (metrics.py:389-415).  on_device: the files
    become MatchTables and the segment AP is computed by libvscmi (`match_metric_table`): the same values, bit for bit."""
    if on_device:
        truth_t = MatchTable.read_csv(ground_truth_filename, is_gt=True)
        predicted_t = MatchTable.read_csv(predictions_filename)
        return MatchingTrackMetrics(segment_ap=match_metric_table(truth_t, predicted_t),
                                    pairwise_micro_ap=pairwise_ap_table(truth_t, predicted_t))
    truth = Match.read_csv(ground_truth_filename, is_gt=True)
    predicted = Match.read_csv(predictions_filename)
    pair_ap = average_precision(CandidatePair.from_matches(truth), CandidatePair.from_matches(predicted))
    return MatchingTrackMetrics(segment_ap=match_metric(truth, predicted), pairwise_micro_ap=pair_ap)


def average_precision(ground_truth: Collection[CandidatePair], predictions: Collection[CandidatePair]
                      ) -> AveragePrecision:
    """Micro-AP over (query, ref) pairs (metrics.py:418-450): `ap` is the DrivenData value
    (threshold-grouped AP scaled by the share of the ground truth that was predicted at all),
    `simple_ap` the rank-based one."""
    gq, gr, _ = _pair_columns(ground_truth)
    wanted = set(zip(gq, gr))
    if len(wanted) != len(gq):
        raise AssertionError("Duplicates detected in ground truth")
    pq, pr, scores = _pair_columns(predictions)
    if len(set(zip(pq, pr))) != len(pq):
        raise AssertionError("Duplicates detected in predictions")
    canonical = drivendata_average_precision(predicted=CandidatePair.to_dataframe(predictions),
                                             ground_truth=CandidatePair.to_dataframe(ground_truth))
    order = np.argsort(-scores, kind="stable")
    hit = np.fromiter(((pq[k], pr[k]) in wanted for k in order), dtype=bool, count=len(order))
    found = np.cumsum(hit)
    precision = found / (np.arange(len(hit)) + 1)
    recall = found / len(wanted)
    simple_ap = np.sum(precision * hit) / len(wanted)
    at = np.flatnonzero(hit)
    return AveragePrecision(ap=canonical, pr_curve=PrecisionRecallCurve(precision[at], recall[at], scores[order][at]),
                            simple_ap=simple_ap)


def _threshold_ap(labels: np.ndarray, scores: np.ndarray) -> float:
    """Binary average precision as sklearn.metrics.average_precision_score defines it: over the
    distinct score thresholds, descending, sum (R_k - R_{k-1}) * P_k."""
    order = np.argsort(-scores, kind="stable")
    labels, scores = labels[order], scores[order]
    group_end = np.r_[np.flatnonzero(np.diff(scores)), len(scores) - 1]
    tp = np.cumsum(labels)[group_end]
    precision = tp / (group_end + 1)
    recall = tp / tp[-1]
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def drivendata_average_precision(predicted, ground_truth) -> float:
    """The challenge backend's AP (metrics.py:453-489); both arguments are frames with query_id /
    ref_id (/ score) columns."""
    if len(predicted) == 0:
        return 0.0
    scores = np.asarray(predicted["score"], dtype=np.float64)
    if not np.isfinite(scores).all():
        raise ValueError("Scores must be finite.")
    truth = set(zip(ground_truth["query_id"], ground_truth["ref_id"])) if len(ground_truth) else set()
    labels = np.fromiter((pair in truth for pair in zip(predicted["query_id"], predicted["ref_id"])),
                         dtype=np.float64, count=len(scores))
    n_found = int(labels.sum())
    if n_found == 0:
        return 0.0
    n_truth = int(_pandas().notna(ground_truth["ref_id"]).sum())
    return _threshold_ap(labels, scores) * (n_found / n_truth)
