"""The pre-filters' error bounds at the inputs that come closest to them (tests/prefilter_bounds.py).

Every other pre-filter test runs on random or descriptor-like rows, whose rounding errors mostly cancel: there the real
error of the fp16 and int8 scores stays at a fraction of the bound, and a bound several times too tight would go
unnoticed.  Here the planted pairs' rounding errors all point the same way (int8: >= 0.97 of eps; fp16: 0.79-0.97 of
c1 |q||r|) and each planted pair meets its threshold so closely that a bound of 0.9 eps would drop it (fp16 at
D >= 512: the construction's reach, 0.85 / 0.75 eps).  Every route is forced with handle options -- fp16 panel, fp16
LDS ring, int8 with single and paired work items, int8 with an excluded coordinate, with a centred reference image,
with the fp16 screen -- and every query kind meets the bound: the range search at radius nextafter(s, -inf), the global
top-K with the radius
of its first batch just below the planted score, the k-NN (k = 1, 5) with the partner at rank k behind a threshold just
below it (the non-strict per-row path).  Results must equal the CPU oracle bit for bit, hold every planted pair, and
come from the intended kernel.
"""
import numpy as np
import pytest

import prefilter_bounds as pb


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# route -> (handle options, kind of construction, dimension, construction options)
ROUTES = {
    "f16-panel-64": (dict(prefilter=2, i8=0), "f16", 64, {}),
    "f16-panel-512": (dict(prefilter=2, i8=0), "f16", 512, {}),
    "f16-ring-768": (dict(prefilter=2, i8=0, f16_kernel=1), "f16", 768, {}),
    "f16-ring-1000": (dict(prefilter=2, i8=0, f16_kernel=1), "f16", 1000, {}),
    "i8-64": (dict(prefilter=2, i8=2, i8p_pair=0), "i8", 64, {}),
    "i8-512": (dict(prefilter=2, i8=2, i8p_pair=0), "i8", 512, {}),
    "i8-1000": (dict(prefilter=2, i8=2, i8p_pair=0), "i8", 1000, {}),
    "i8-pair-64": (dict(prefilter=2, i8=2, i8p_pair=2), "i8", 64, {}),
    "i8-pair-512": (dict(prefilter=2, i8=2, i8p_pair=2), "i8", 512, {}),
    "i8-excluded-128": (dict(prefilter=2, i8=2), "i8", 128, dict(exclude=True)),
    "i8-centred-256": (dict(prefilter=2, i8=2, i8_center=2), "i8", 256, dict(centre=True)),
    "i8-screen-512": (dict(prefilter=2, i8=2, i8_screen=1), "i8", 512, {}),
}


def case(route, query):
    _, kind, d, kw = ROUTES[route]
    if query == "topk":
        return pb.topk_case(kind, d, **kw)
    return pb.knn_case(kind, d, int(query[3:]), **kw)


def index(route, c):
    from vsc2022_amd.vsc.index import FlatIndex

    idx = FlatIndex(c.d, options={k: float(v) for k, v in ROUTES[route][0].items()})
    idx.profile(True)
    idx.add(c.r)
    return idx


def chain_scores(orc, q, r):
    """the oracle's fp32 chain score of every pair (q[n], r[n])"""
    return np.array([orc.scores(q[n : n + 1], r[n : n + 1])[0, 0] for n in range(len(q))], dtype=np.float32)


def one_score(orc, c, rows, refs):
    """all pairs of a role share one chain score (the same products in the same order)"""
    s = chain_scores(orc, c.q[rows[[0, -1]]], c.r[refs[[0, -1]]])
    assert s[0] == s[1], s
    return s[0]


def assert_teeth(c, rows, refs, t):
    """the planted pairs meet threshold t (the whole score's) within the reach of the construction: a bound f eps
    (f = 0.9 for int8, the dimension's fp16 reach) would lose them, eps keeps them"""
    b = pb.PairBound(c, rows, refs)
    m = b.margin(t)
    f = pb.I8_MARGIN if c.kind == "i8" else min(pb.I8_MARGIN, pb.F16_REACH[c.d])
    assert (m > f).all() and (m < 1.0).all(), (m.min(), m.max(), f)


def assert_route(route, idx, st):
    if ROUTES[route][1] == "i8":
        assert st["i8_launches"] > 0 and idx.get_option("i8_fallbacks") == 0, st
    else:
        assert st["f16_launches"] > 0 and st["i8_launches"] == 0, st
    if ROUTES[route][3].get("centre"):
        assert idx.get_option("i8_center_on") == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_range_search_at_the_bound(gpu, orc, route):
    c = case(route, "topk")
    rows, refs = c.planted()
    s = one_score(orc, c, rows, refs)
    radius = np.nextafter(s, np.float32(-np.inf))
    assert_teeth(c, rows, refs, radius)
    idx = index(route, c)
    lims, D, I = idx.range_search(c.q, radius)
    st = idx.profile_read(reset=True)
    ol, oD, oI = orc.range_search(c.q, c.r, radius)
    # the hits are exactly the planted pairs (one per row after the first 32)
    assert np.array_equal(np.diff(ol.astype(np.int64)), (c.partner >= 0).astype(np.int64)) and np.array_equal(oI, refs)
    assert np.array_equal(lims, ol) and np.array_equal(I, oI)
    assert np.array_equal(bits(D), bits(oD))
    assert_route(route, idx, st)


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_global_topk_at_the_bound(gpu, orc, route):
    c = case(route, "topk")
    rows, refs = c.planted()
    s_d = chain_scores(orc, c.q[:1], pb.decoys(c, np.arange(1)))[0]   # (the first batch's rows hold the decoys)
    assert s_d < one_score(orc, c, rows, refs)
    assert_teeth(c, rows, refs, s_d)
    idx = index(route, c)
    i, j, s, radius = idx.global_topk(c.q, c.K)
    st = idx.profile_read(reset=True)
    oi, oj, os_, info = orc.global_threshold_search(c.q, c.r, c.K, 0, return_info=True)
    # the first batch's decoys set the radius just below the planted score; the K results are the planted pairs
    assert np.float32(info["radius"]) == s_d and np.array_equal(oi, rows) and np.array_equal(oj, refs)
    assert len(s) == len(os_)
    assert np.array_equal(i, oi) and np.array_equal(j, oj) and np.array_equal(bits(s), bits(os_))
    assert np.float32(radius) == np.float32(info["radius"])
    assert_route(route, idx, st)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("route", list(ROUTES))
def test_knn_at_the_bound(gpu, orc, route, k):
    c = case(route, f"knn{k}")
    rows, refs = c.planted()
    s = one_score(orc, c, rows, refs)
    s_d = chain_scores(orc, c.q[rows[:1]], pb.decoys(c, rows[:1]))[0]
    assert s_d < s
    assert_teeth(c, rows, refs, s_d)
    idx = index(route, c)
    D, I = idx.search(c.q, k)
    st = idx.profile_read(reset=True)
    oD, oI = orc.knn(c.q, c.r, k)
    # the partner is rank k, the decoy (rank k + 1) holds the threshold its range is searched with
    assert np.array_equal(oI[:, k - 1], refs) and (oD[:, k - 1] == s).all()
    assert np.array_equal(I, oI) and np.array_equal(bits(D), bits(oD))
    assert_route(route, idx, st)
