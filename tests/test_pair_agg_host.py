"""CPU: the host statement of the sum / mean / top-m mean aggregations (vsc2022_amd/vsc/candidates.py) against the
restatement of tests/pair_agg_ref.py, the dispatch predicate of CandidateGeneration.query, and the C ABI's constants,
exports and argument checks (which come before any device is looked at)."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import bits
from pair_agg_ref import aggregate_run, pair_aggregate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# descending float64 sums give 0.0 on these, list order / blocked / tree sums something else
ORDER_RUNS = [
    [2.0 ** 53] + [1.0] * 64 + [-(2.0 ** 53)],
    [1.0] * 64 + [-(2.0 ** 53), 2.0 ** 53],
    [1e30, -1e30, 1.0],
    [1.0, -1e30, 1e30],
]


def _match(scores, view):
    from vsc2022_amd.vsc.index import PairMatch, PairMatches, VideoMetadata, _MatchView

    scores = np.asarray(scores, dtype=np.float32)
    if view:
        meta = VideoMetadata("v", np.arange(len(scores), dtype=np.float32))
        idx = np.arange(len(scores))
        return PairMatches("q", "r", _MatchView(meta, meta, idx, idx, scores))
    return PairMatches("q", "r", [PairMatch((0.0, 0.0), (0.0, 0.0), s) for s in scores])


def _runs():
    rng = np.random.default_rng(5)
    runs = [rng.standard_normal(n).astype(np.float32) for n in (1, 2, 3, 63, 64, 65, 257, 1000)]
    runs += [(rng.integers(-8, 9, 40) / 8).astype(np.float32), np.array([0.0, -0.0, 0.0], np.float32),
             np.array([-0.0, -0.0], np.float32), np.array([3e38, 3e38, -1.0], np.float32),
             np.array([1e-45, -1e-45, 1e-45], np.float32)]
    runs += [np.array(r, dtype=np.float32) for r in ORDER_RUNS]
    return runs


@pytest.mark.parametrize("view", [False, True])
def test_host_classes_equal_the_restatement(view):
    from vsc2022_amd.vsc.candidates import MeanScoreAggregation, SumScoreAggregation, TopMeanScoreAggregation

    for run in _runs():
        m = _match(run, view)
        cases = [(SumScoreAggregation(), "sum", 1), (MeanScoreAggregation(), "mean", 1)]
        cases += [(TopMeanScoreAggregation(k), "topmean", k) for k in (1, 2, 3, 65, 66, 10 ** 6)]
        for agg, name, k in cases:
            with np.errstate(over="ignore"):
                got = agg.aggregate(m)
            assert isinstance(got, np.float32), (name, type(got))
            assert bits(got) == bits(aggregate_run(run, name, k)), (name, k, run[:4], got)
            assert agg.score(m).score is got or bits(agg.score(m).score) == bits(got)


def test_order_revealing_runs_sum_to_zero_only_in_descending_order():
    from vsc2022_amd.vsc.candidates import MeanScoreAggregation, SumScoreAggregation, TopMeanScoreAggregation

    for run in ORDER_RUNS:
        m = _match(run, False)
        assert SumScoreAggregation().aggregate(m) == 0.0 and MeanScoreAggregation().aggregate(m) == 0.0
        assert TopMeanScoreAggregation(len(run)).aggregate(m) == 0.0
        assert aggregate_run(run, "sum") == 0.0
    # ... and the same runs summed in list order do not: the runs do reveal the order
    assert float(np.cumsum(np.array(ORDER_RUNS[1], dtype=np.float64))[-1]) == 64.0
    assert float(np.cumsum(np.array(ORDER_RUNS[2], dtype=np.float64))[-1]) == 1.0


def test_topmean_1_is_max_and_m_beyond_the_run_is_mean():
    from vsc2022_amd.vsc.candidates import MaxScoreAggregation, MeanScoreAggregation, TopMeanScoreAggregation

    rng = np.random.default_rng(6)
    for n in (1, 5, 64, 300):
        run = rng.standard_normal(n).astype(np.float32)
        m = _match(run, True)
        assert bits(TopMeanScoreAggregation(1).aggregate(m)) == bits(MaxScoreAggregation().aggregate(m))
        assert bits(TopMeanScoreAggregation(n).aggregate(m)) == bits(MeanScoreAggregation().aggregate(m))
        assert bits(TopMeanScoreAggregation(n + 7).aggregate(m)) == bits(MeanScoreAggregation().aggregate(m))


@pytest.mark.parametrize("m", [0, -1, 1.5])
def test_top_m_below_one_raises(m):
    from vsc2022_amd.vsc.candidates import TopMeanScoreAggregation

    with pytest.raises(ValueError):
        TopMeanScoreAggregation(m)


def test_restatement_orders_pairs_by_first_appearance_then_score():
    row2q = np.array([0, 0, 1], np.int32)
    row2r = np.array([0, 0, 1, 2], np.int32)
    i = np.array([2, 0, 1, 0, 2], np.int32)
    j = np.array([3, 0, 1, 3, 0], np.int32)
    s = np.array([0.5, 0.25, 0.25, 0.5, 0.125], np.float32)
    q, r, sc, first, cnt = pair_aggregate_ref(i, j, s, row2q, row2r, "sum")
    # pairs in list order: (1,2) 0.5 | (0,0) 0.25 | (0,0) 0.25 | (0,2) 0.5 | (1,0) 0.125
    assert list(zip(q, r)) == [(1, 2), (0, 0), (0, 2), (1, 0)]
    assert sc.tolist() == [0.5, 0.5, 0.5, 0.125] and first.tolist() == [0, 1, 3, 4] and cnt.tolist() == [1, 2, 1, 1]


def test_only_exact_types_take_the_device_route():
    from vsc2022_amd import _lib
    from vsc2022_amd.vsc import candidates as C

    assert C.device_aggregation(C.MaxScoreAggregation()) == (_lib.AGG_MAX, 1)
    assert C.device_aggregation(C.SumScoreAggregation()) == (_lib.AGG_SUM, 1)
    assert C.device_aggregation(C.MeanScoreAggregation()) == (_lib.AGG_MEAN, 1)
    assert C.device_aggregation(C.TopMeanScoreAggregation(7)) == (_lib.AGG_TOPMEAN, 7)

    class User(C.ScoreAggregation):
        def aggregate(self, match):
            return 0.0

    subclasses = [type("Sub", (cls,), {}) for cls in (C.MaxScoreAggregation, C.SumScoreAggregation, C.MeanScoreAggregation)]
    for agg in [User()] + [cls() for cls in subclasses] + [type("SubTop", (C.TopMeanScoreAggregation,), {})(3)]:
        assert C.device_aggregation(agg) is None
        for K in (100, 0, -2):
            assert C.device_route(agg, K, 50) is None
    # max with a global threshold keeps its own entry point; everything else built in goes to the new one
    assert C.device_route(C.MaxScoreAggregation(), 100, 50) == "max"
    assert C.device_route(C.MaxScoreAggregation(), -5, 50) == ("agg", _lib.AGG_MAX, 1)
    assert C.device_route(C.SumScoreAggregation(), 100, 50) == ("agg", _lib.AGG_SUM, 1)
    assert C.device_route(C.TopMeanScoreAggregation(4), -50, 50) == ("agg", _lib.AGG_TOPMEAN, 4)
    # k beyond the reference rows: the generic route (an empty slot has no video)
    assert C.device_route(C.SumScoreAggregation(), -51, 50) is None
    assert C.device_route(C.MaxScoreAggregation(), -51, 50) is None


def test_header_constants_exports_and_argtypes():
    from vsc2022_amd import _lib

    header = open(os.path.join(ROOT, "include", "vscmi.h")).read()
    value = {k: int(v) for k, v in re.findall(r"#define (VSC_AGG_[A-Z_]+) (\d+)\b", header)}
    assert value == {"VSC_AGG_MAX": _lib.AGG_MAX, "VSC_AGG_SUM": _lib.AGG_SUM, "VSC_AGG_MEAN": _lib.AGG_MEAN,
                     "VSC_AGG_TOPMEAN": _lib.AGG_TOPMEAN}
    assert (_lib.AGG_MAX, _lib.AGG_SUM, _lib.AGG_MEAN, _lib.AGG_TOPMEAN) == (0, 1, 2, 3)
    declared = set(re.findall(r"\b(vsc_[a-z0-9_]+)\s*\(", header))
    for name in ("vsc_pair_aggregate", "vsc_index_candidates_agg"):
        assert name in declared and name in _lib.EXPORTS
    L = _lib.lib()
    assert len(L.vsc_pair_aggregate.argtypes) == len(L.vsc_pair_max.argtypes) + 4  # hits_order, agg, top_m, out_count
    assert len(L.vsc_index_candidates_agg.argtypes) == len(L.vsc_index_candidates.argtypes) + 2
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`vsc_pair_aggregate`" in doc and "`vsc_index_candidates_agg`" in doc


@pytest.mark.parametrize("agg,top_m", [(4, 1), (-1, 1), (3, 0), (3, -5)])
def test_bad_aggregation_is_refused_before_any_device(agg, top_m):
    from vsc2022_amd import _lib

    L = _lib.lib()
    z32, zf = np.zeros(4, np.int32), np.zeros(4, np.float32)
    out = [np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.float32), np.zeros(4, np.int64), np.zeros(4, np.int32)]
    n_pairs = ctypes.c_int64(-7)
    # device ordinal 10 ** 6 does not exist anywhere: an answer of VSC_ERR_INVALID about the aggregation came first
    rc = L.vsc_pair_aggregate(z32.ctypes.data, z32.ctypes.data, zf.ctypes.data, 4, _lib.MEM_HOST, z32.ctypes.data, 4,
                              z32.ctypes.data, 4, _lib.MEM_HOST, 1, agg, top_m, *[o.ctypes.data for o in out], 4,
                              _lib.MEM_HOST, ctypes.byref(n_pairs), 10 ** 6)
    assert rc == _lib.VSC_ERR_INVALID
    msg = L.vsc_last_error().decode()
    assert "aggregation" in msg or "top_m" in msg, msg
    # the index form judges the aggregation before it looks at its handle
    rc = L.vsc_index_candidates_agg(None, None, 0, _lib.MEM_HOST, 10, None, None, agg, top_m, None, None, None, 0,
                                    ctypes.byref(n_pairs), None)
    assert rc == _lib.VSC_ERR_INVALID
    msg = L.vsc_last_error().decode()
    assert "aggregation" in msg or "top_m" in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_host_hits_out_of_range_are_refused_on_the_host():
    from vsc2022_amd import _lib

    L = _lib.lib()
    maps = np.zeros(4, np.int32)
    zf = np.zeros(3, np.float32)
    out = [np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.float32)]
    n_pairs = ctypes.c_int64(0)
    for hi, hj in (([0, 4, 0], [0, 0, 0]), ([0, 0, 0], [0, 0, -1])):
        hi, hj = np.array(hi, np.int32), np.array(hj, np.int32)
        rc = L.vsc_pair_aggregate(hi.ctypes.data, hj.ctypes.data, zf.ctypes.data, 3, _lib.MEM_HOST, maps.ctypes.data, 4,
                                  maps.ctypes.data, 4, _lib.MEM_HOST, 0, _lib.AGG_SUM, 1, *[o.ctypes.data for o in out],
                                  None, None, 3, _lib.MEM_HOST, ctypes.byref(n_pairs), 10 ** 6)
        assert rc == _lib.VSC_ERR_INVALID and "outside" in L.vsc_last_error().decode()


def test_engine_aggregation_names():
    from vsc2022_amd import _lib
    from vsc2022_amd.engine import aggregation_id

    assert aggregation_id("max") == (_lib.AGG_MAX, 1) and aggregation_id("sum") == (_lib.AGG_SUM, 1)
    assert aggregation_id("mean") == (_lib.AGG_MEAN, 1) and aggregation_id(("topmean", 5)) == (_lib.AGG_TOPMEAN, 5)
    assert aggregation_id(_lib.AGG_TOPMEAN, 3) == (_lib.AGG_TOPMEAN, 3)
    for bad in ("median", ("topmean", 0), ("topmean",), ("sum", 2), 9):
        with pytest.raises(ValueError):
            aggregation_id(bad)
