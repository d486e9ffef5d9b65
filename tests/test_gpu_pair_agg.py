"""GPU: vsc_pair_aggregate / vsc_index_candidates_agg (csrc/pair_reduce.hip) against the restatement of
tests/pair_agg_ref.py on every output column (q, r, score BITS, first, count), for every aggregation, both hit orders
and host and device memory; the device route of CandidateGeneration.query against the generic route; k-NN + max against
the committed goldens; DeviceMatcher.match(aggregation=...); the refusals.

The shapes are the smallest at which the kernels can go wrong: run lengths around the wave (63 / 64 / 65) and the
workgroup (255 / 256 / 257), one long run (1000, 5000), a run across a 256-lane boundary of the head detection, one hit,
all hits in distinct pairs, and scores on a 1/8 grid so that many pairs tie on the aggregated score and the stable
first-appearance order decides.  Random data cannot catch a wrong summation order (descending and ascending float64 sums
rounded to fp32 agree on random runs), so runs are planted whose float64 sum is 0.0 in descending order only.
The largest case holds 20 000 hits."""
import ctypes
import logging

import numpy as np
import pytest

from helpers import bits, load, videos
from pair_agg_ref import CASES, pair_aggregate_ref
from pair_agg_ref import assert_columns as _assert_columns
from pair_agg_ref import case as _case

pytestmark = pytest.mark.gpu

AGGS = [("max", 1), ("sum", 1), ("mean", 1), ("topmean", 2), ("topmean", 65), ("topmean", 66)]


def _agg_id(name):
    from vsc2022_amd import _lib

    return {"max": _lib.AGG_MAX, "sum": _lib.AGG_SUM, "mean": _lib.AGG_MEAN, "topmean": _lib.AGG_TOPMEAN}[name]


def _device_call(i, j, s, row2q, row2r, agg, m, hits_order, device_mem):
    from vsc2022_amd import _lib

    n = len(s)
    if device_mem:
        import torch

        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (i, j, s, row2q, row2r)]
        out = [torch.empty(n, dtype=d, device=dev) for d in (torch.int32, torch.int32, torch.float32, torch.int64, torch.int32)]
        torch.cuda.synchronize(dev)
        ptr = [a.data_ptr() for a in t]
        optr = [a.data_ptr() for a in out]
        mem = _lib.MEM_DEVICE
    else:
        t = [np.ascontiguousarray(a) for a in (i, j, s, row2q, row2r)]
        out = [np.empty(n, dtype=d) for d in (np.int32, np.int32, np.float32, np.int64, np.int32)]
        ptr = [a.ctypes.data for a in t]
        optr = [a.ctypes.data for a in out]
        mem = _lib.MEM_HOST
    n_pairs = ctypes.c_int64(0)
    _lib.check(_lib.lib().vsc_pair_aggregate(ptr[0], ptr[1], ptr[2], n, mem, ptr[3], len(row2q), ptr[4], len(row2r), mem,
                                             hits_order, _agg_id(agg), m, *optr, n, mem, ctypes.byref(n_pairs), 0))
    k = n_pairs.value
    return tuple((a.cpu().numpy() if device_mem else a)[:k] for a in out)


@pytest.mark.parametrize("hits_order", [1, 0])
@pytest.mark.parametrize("case", CASES)
def test_every_column_equals_the_restatement(gpu, case, hits_order):
    i, j, s, row2q, row2r = _case(case)
    if not hits_order:  # any order: a random permutation of the same hits
        perm = np.random.default_rng(3).permutation(len(s))
        i, j, s = i[perm], j[perm], s[perm]
    else:
        assert np.all(s[:-1] >= s[1:])
    for agg, m in AGGS:
        with np.errstate(over="ignore"):
            exp = pair_aggregate_ref(i, j, s, row2q, row2r, agg, m)
        for device_mem in (False, True):
            got = _device_call(i, j, s, row2q, row2r, agg, m, hits_order, device_mem)
            _assert_columns(got, exp, (case, agg, m, hits_order, "device" if device_mem else "host"))
    if case == "order_revealing":
        q, r, sc, _, _ = pair_aggregate_ref(i, j, s, row2q, row2r, "sum")
        planted = {(int(a), int(b)): float(v) for a, b, v in zip(q, r, sc) if a == 7}
        assert planted == {(7, 0): 0.0, (7, 1): 0.0, (7, 2): 0.0, (7, 3): 0.0}  # (list order: 64, 1.0, 300, 0.25)
    if case == "quantised":
        sc = pair_aggregate_ref(i, j, s, row2q, row2r, "sum")[2]
        assert len(sc) - len(np.unique(sc)) > 100  # many pairs do tie on the aggregated score


def test_order_revealing_expectations_are_what_descending_order_gives():
    """(no device) the planted runs: 0.0 in descending order, 64 / 1.0 in other orders"""
    from pair_agg_ref import aggregate_run

    assert aggregate_run([1.0] * 64 + [-(2.0 ** 53), 2.0 ** 53], "sum") == 0.0
    assert aggregate_run([1.0, -1e30, 1e30], "sum") == 0.0 and aggregate_run([1.0, 1e30, -1e30, 0.25], "sum") == 0.0
    assert float(np.float64(np.float32(1e30)) - np.float64(np.float32(1e30)) + 1.0) == 1.0
    acc = 0.0
    for v in [1.0] * 64 + [-(2.0 ** 53), 2.0 ** 53]:
        acc += v
    assert acc == 64.0


# ------------------------------------------------------------------ the public surface

def _planted():
    from vsc2022_amd import synth
    from vsc2022_amd.vsc.index import VideoFeature

    q, r, _ = synth.make_dataset(seed=31, n_query=12, n_ref=15, dim=64, q_frames=(20, 30), r_frames=(20, 30), planted_frac=0.5,
                                 noise=0.05, copy_len=(8, 20))
    return synth.to_video_features(q, VideoFeature), synth.to_video_features(r, VideoFeature)


def _builtin(name):
    from vsc2022_amd.vsc import candidates as C

    return {"max": (C.MaxScoreAggregation, ()), "sum": (C.SumScoreAggregation, ()), "mean": (C.MeanScoreAggregation, ()),
            "topmean3": (C.TopMeanScoreAggregation, (3,))}[name]


@pytest.mark.parametrize("global_k", [3000, -8])
@pytest.mark.parametrize("name", ["max", "sum", "mean", "topmean3"])
def test_device_route_equals_the_generic_route(gpu, name, global_k, caplog):
    from vsc2022_amd.vsc.candidates import CandidateGeneration, CandidateList
    from vsc2022_amd.vsc.index import KNN_WARNING

    q, r = _planted()
    cls, args = _builtin(name)

    class User(cls):
        pass

    with caplog.at_level(logging.WARNING):
        dev = CandidateGeneration(r, cls(*args)).query(q, global_k)
    assert (KNN_WARNING in caplog.text) == (global_k < 0)
    cg = CandidateGeneration(r, User(*args))
    gen = cg.query(q, global_k)
    n_hits = sum(len(pm.matches) for pm in cg.index.search(q, global_k))
    assert isinstance(dev, CandidateList) and isinstance(gen, list)  # the two routes, not one twice
    assert len(gen) >= 50 and n_hits >= 2000, (len(gen), n_hits)
    assert len(dev) == len(gen)
    assert [c.query_id for c in dev] == [c.query_id for c in gen] and [c.ref_id for c in dev] == [c.ref_id for c in gen]
    assert np.array_equal(bits([c.score for c in dev]), bits([c.score for c in gen]))
    assert all(isinstance(c.score, np.float32) for c in gen[:5])


@pytest.mark.parametrize("case", ["g2_search_plain", "g2_search_ties", "g2_search_d512"])
def test_knn_max_equals_the_reference(gpu, case):
    """the reference's own k-NN PairMatches (goldens) -> per-pair max -> its stable descending sort"""
    from vsc2022_amd.vsc.candidates import CandidateGeneration, CandidateList, MaxScoreAggregation
    from vsc2022_amd.vsc.index import VideoFeature

    fx = load(case)
    q, r = videos(fx, "q", VideoFeature), videos(fx, "r", VideoFeature)
    cg = CandidateGeneration(r, MaxScoreAggregation())
    checked = 0
    for k in fx["knn_ks"]:
        pq, pr, pn, sc = fx[f"knn{k}_pm_q"], fx[f"knn{k}_pm_r"], fx[f"knn{k}_pm_n"], fx[f"knn{k}_pm_score32"]
        cuts = np.r_[0, np.cumsum(pn)]
        best = [np.max(sc[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        order = sorted(range(len(best)), key=lambda p: best[p], reverse=True)
        got = cg.query(q, -int(k))
        assert isinstance(got, CandidateList)
        assert [c.query_id for c in got] == [str(pq[p]) for p in order]
        assert [c.ref_id for c in got] == [str(pr[p]) for p in order]
        assert np.array_equal(bits([c.score for c in got]), bits([best[p] for p in order]))
        checked += len(order)
    assert checked > 0


def _matcher():
    import torch

    from vsc2022_amd import engine, synth

    dev = torch.device("cuda", 0)
    n_qv, qf, n_rv, rf, dim = 20, 10, 30, 10, 64
    refs = synth.device_rows(torch, dev, 5, n_rv, rf, dim)
    queries = synth.device_rows(torch, dev, 6, n_qv, qf, dim)
    m = engine.DeviceMatcher(refs, np.arange(n_rv + 1, dtype=np.int64) * rf, 0)
    m.set_queries(queries, np.arange(n_qv + 1, dtype=np.int64) * qf)
    return m


def test_matcher_sum_is_pair_aggregate_of_its_hits(gpu):
    m = _matcher()
    res = m.match(localize=False, aggregation="sum")
    hi, hj, hs = m.last_hits
    assert res.n_hits == hs.numel() == 1200 * 20
    i, j, s = hi.cpu().numpy(), hj.cpu().numpy(), hs.cpu().numpy()
    exp = pair_aggregate_ref(i, j, s, m.row2q.cpu().numpy(), m.row2r.cpu().numpy(), "sum")
    got = tuple(t.cpu().numpy() for t in m.pair_aggregate(hi, hj, hs, "sum"))
    _assert_columns(got, exp, "pair_aggregate")
    n = res.n_candidates
    assert 0 < n <= len(exp[0]) and res.n_pairs == len(exp[0])
    assert np.array_equal(res.cand_q.cpu().numpy(), exp[0][:n]) and np.array_equal(res.cand_r.cpu().numpy(), exp[1][:n])
    assert np.array_equal(bits(res.cand_score.cpu().numpy()), bits(exp[2][:n]))
    # ... and differs from the max table: the argument does something
    assert not np.array_equal(bits(m.match(localize=False).cand_score.cpu().numpy()), bits(exp[2][:n]))


def test_matcher_max_is_the_default_call(gpu):
    import torch

    m = _matcher()
    a = m.match()
    a = {k: getattr(a, k).clone() for k in ("cand_q", "cand_r", "cand_score", "nbox", "boxes", "box_score")}
    b = m.match(aggregation="max")
    for k, v in a.items():
        assert torch.equal(v, getattr(b, k)), k
    with pytest.raises(ValueError):
        m.match(aggregation="median")
    with pytest.raises(ValueError):
        m.match(aggregation=("topmean", 0))


# ------------------------------------------------------------------ refusals

def test_knn_beyond_the_reference_rows_stays_generic(gpu):
    from vsc2022_amd.vsc.candidates import CandidateGeneration, SumScoreAggregation
    from vsc2022_amd.vsc.index import VideoFeature

    rng = np.random.default_rng(8)

    def vids(prefix, n):
        return [VideoFeature(video_id=f"{prefix}{k}", timestamps=np.arange(2, dtype=np.float32),
                             feature=rng.standard_normal((2, 16)).astype(np.float32)) for k in range(n)]

    q, r = vids("Q", 3), vids("R", 3)

    class User(SumScoreAggregation):
        pass

    at = CandidateGeneration(r, SumScoreAggregation()).query(q, -6)  # k == ntotal: still the device route
    assert not isinstance(at, list) and at == CandidateGeneration(r, User()).query(q, -6)
    with np.errstate(over="ignore"):  # (the empty slots carry -FLT_MAX: their float64 sums leave fp32)
        beyond = CandidateGeneration(r, SumScoreAggregation()).query(q, -7)
        assert isinstance(beyond, list)
        assert beyond == CandidateGeneration(r, User()).query(q, -7)


def test_candidates_agg_refuses_k_beyond_ntotal(gpu):
    from vsc2022_amd import _lib
    from vsc2022_amd.vsc.index import FlatIndex

    idx = FlatIndex(16)
    idx.add(np.eye(16, dtype=np.float32)[:5])
    q = np.eye(16, dtype=np.float32)[:2]
    maps = np.zeros(5, np.int32)
    out = [np.zeros(16, np.int32), np.zeros(16, np.int32), np.zeros(16, np.float32)]
    n_pairs, n_hits = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = _lib.lib().vsc_index_candidates_agg(idx.handle, q.ctypes.data, 2, _lib.MEM_HOST, -6, maps.ctypes.data, maps.ctypes.data,
                                             _lib.AGG_SUM, 1, *[o.ctypes.data for o in out], 16, ctypes.byref(n_pairs),
                                             ctypes.byref(n_hits))
    assert rc == _lib.VSC_ERR_INVALID and n_hits.value == 0


@pytest.mark.parametrize("hits_order", [1, 0])
def test_device_hit_rows_out_of_range_raise(gpu, hits_order):
    i, j, s, row2q, row2r = _case("run_lengths")
    for arr, bad in ((i, len(row2q)), (j, -1)):
        keep = arr[700]
        arr[700] = bad
        with pytest.raises(ValueError, match="outside"):
            _device_call(i, j, s, row2q, row2r, "sum", 1, hits_order, True)
        arr[700] = keep
    # the context is usable afterwards
    exp = pair_aggregate_ref(i, j, s, row2q, row2r, "mean")
    _assert_columns(_device_call(i, j, s, row2q, row2r, "mean", 1, 1, True), exp, "after a refusal")
