"""Every device implementation of the fp32 chain `acc = fmaf(q[k], r[k], acc)` against the CPU oracle, bit for bit, on
the input classes of tests/chain_cases.py: subnormal operands, subnormal sums, products that underflow to +-0, chains
that overflow half-way (+-inf, inf - inf = NaN), cancellations, and all of them mixed with ordinary rows in one tile.
tests/test_chain_contract_host.py pins the oracle itself (against an exact integer restatement) and the classes.

Routes, all forced with handle options: the exact MFMA kernels (prefilter = 0), the VALU exact stage behind the fp16 and
the int8 pre-filter (with deferral 1 and 2 on top), the generic score matrix (L2; inner product with k = 70), the SQfp16
store (`score_matrix_h16`, its exact stage, the half-float Temporal Network tile), the Temporal Network / aligner tile
with the aligners behind it, and `vsc_row_normalize`.

What is compared: a range search at radius -inf returns every pair whose score is neither NaN nor -inf (the comparison
is strict), in (row, reference) order, with the oracle's bits -- the sign of a zero included; thresholded range search,
global top-K (hits, order, score bits, radius) and k-NN (on the inputs without the NaN-producing rows: the reference leaves
the order over NaN undefined) equal the oracle's.  NaN payloads are not part of the contract.
"""
import functools

import numpy as np
import pytest

import chain_cases as cc
from codec_rows import dec
from helpers import bits

pytestmark = pytest.mark.gpu

CASES = [(name, d) for name in cc.CLASSES for d in cc.DIMS]
IDS = [f"{name}-{d}" for name, d in CASES]
EXACT = dict(prefilter=0)
PREFILTER_ROUTES = {
    "f16": dict(prefilter=2, i8=0), "i8": dict(prefilter=2, i8=2),
    "f16-defer1": dict(prefilter=2, i8=0, defer=1), "f16-defer2": dict(prefilter=2, i8=0, defer=2),
    "i8-defer1": dict(prefilter=2, i8=2, defer=1), "i8-defer2": dict(prefilter=2, i8=2, defer=2),
}
NEG_INF, POS_INF = float("-inf"), float("inf")


# ---------------------------------------------------------------- inputs and oracle results, computed once
@functools.lru_cache(maxsize=None)
def rows(name, d, nr, metric=0, half=False):
    """(q, r, q', r'): the class's rows and the copy without the NaN-producing rows; never modified"""
    if half:
        q, r = cc.fp16_cases(d, cc.NQ, nr)[name]
        r = dec(r)
    elif name == "overflow" and metric == 1:
        q, r = cc.make(name, d, cc.NQ, nr, scale=0.5)
    else:
        q, r = cc.make(name, d, cc.NQ, nr)
    qn, rn = cc.without_nan_rows(q, r)
    for x in (q, r, qn, rn):
        x.setflags(write=False)
    return q, r, qn, rn


@functools.lru_cache(maxsize=None)
def want(kind, name, d, nr, metric=0, half=False, arg=None):
    import oracle as orc

    q, r, qn, rn = rows(name, d, nr, metric, half)
    if kind == "scores":
        return orc.scores(q, r, metric)
    if kind == "range":
        return orc.range_search(q, r, arg, metric)
    if kind == "topk":
        return orc.global_threshold_search(q, r, arg, metric, return_info=True)
    if kind == "knn":
        return orc.knn(qn, rn, arg, metric)
    raise KeyError(kind)


def make_index(d, r, options, metric=0, codec="Flat"):
    from vsc2022_amd.vsc.index import FlatIndex

    idx = FlatIndex(d, metric, options={k: float(v) for k, v in options.items()}, codec=codec)
    idx.profile(True)
    idx.add(r)
    return idx


def check_range(idx, key, q, radius):
    lims, D, I = idx.range_search(q, radius)
    ol, oD, oI = want("range", *key, arg=radius)
    assert np.array_equal(lims, ol), (key, radius, int(lims[-1]), int(ol[-1]))
    assert np.array_equal(I, oI), (key, radius)
    assert np.array_equal(bits(D), bits(oD)), (key, radius, int((bits(D) != bits(oD)).sum()), len(D))
    return len(D)


def check_topk(idx, key, q, K):
    i, j, s, radius = idx.global_topk(q, K)
    oi, oj, os_, info = want("topk", *key, arg=K)
    assert len(s) == len(os_), (key, K, len(s), len(os_), radius, info)
    assert np.array_equal(i, oi) and np.array_equal(j, oj), (key, K, int((i != oi).sum() + (j != oj).sum()))
    assert np.array_equal(bits(s), bits(os_)), (key, K, int((bits(s) != bits(os_)).sum()))
    assert np.float32(radius) == np.float32(info["radius"]), (key, K, radius, info)    # (by value: +-0 are one radius)
    assert int(idx.get_option("n_rethreshold")) == info["n_rethreshold"], (key, K, info)
    return int(idx.get_option("deferred"))


def check_knn(options, key, k, codec="Flat"):
    name, d, nr, metric, half = key
    _, _, qn, rn = rows(*key)
    idx = make_index(d, rn, options, metric, codec)
    D, I = idx.search(qn, k)
    oD, oI = want("knn", *key, arg=k)
    assert np.array_equal(I, oI), (key, k, int((I != oI).sum()))
    assert np.array_equal(bits(D), bits(oD)), (key, k, int((bits(D) != bits(oD)).sum()))
    return idx.profile_read()


def topk_list(name, n_pairs):
    ks = list(cc.topk_cases(name, n_pairs).values())
    if name == "underflow_zero":
        ks.append(n_pairs // 2)       # the cut falls among the zeros: +0.0 and -0.0 tie, (row, reference) order decides
    return ks


def all_searches(options, key, codec="Flat", topk_only=False):
    """range search at -inf (every non-NaN pair, bits), the thresholded range search, the global top-K cases and the
    k-NN of the class on one route; returns the profile of the index the thresholded searches ran on"""
    name, d, nr, metric, half = key
    q, r, qn, rn = rows(*key)
    idx = make_index(d, r, options, metric, codec)
    s = want("scores", *key)
    if not topk_only:
        everything = NEG_INF if metric == 0 else POS_INF
        n = check_range(idx, key, q, everything)
        beyond = (s > everything) if metric == 0 else (s < everything)
        assert n == int(beyond.sum())           # (NaN compares false: never a hit)
        idx.profile_read()
        check_range(idx, key, q, float(cc.range_radius(name, s, metric)))
    deferred = sum(check_topk(idx, key, q, K) for K in topk_list(name, s.size))
    st = idx.profile_read()
    st["deferred"] = deferred           # (of all the top-K searches; the handle's counter is the last search's)
    st["knn"] = [] if topk_only else [check_knn(options, key, k, codec) for k in cc.KNN_KS]
    return st


# ---------------------------------------------------------------- exact MFMA kernels
@pytest.mark.parametrize("name,d", CASES, ids=IDS)
def test_exact_mfma_kernels(gpu, orc, name, d):
    key = (name, d, cc.NR, 0, False)
    q, r, qn, rn = rows(*key)
    st = all_searches(EXACT, key)
    assert st["candidates"] == 0 and st["f16_launches"] == 0 and st["i8_launches"] == 0, st
    # every score of the matrix, through the copy without the NaN-producing rows: nothing but -inf is left out
    s = orc.scores(qn, rn)
    assert not np.isnan(s).any()
    lims, D, I = make_index(d, rn, EXACT).range_search(qn, NEG_INF)
    keep = s > NEG_INF
    assert np.array_equal(np.diff(lims.astype(np.int64)), keep.sum(axis=1))
    assert np.array_equal(I, np.nonzero(keep)[1]) and np.array_equal(bits(D), bits(s[keep]))


# ---------------------------------------------------------------- exact stage (VALU) behind the pre-filters
@pytest.mark.parametrize("route", list(PREFILTER_ROUTES))
@pytest.mark.parametrize("name,d", CASES, ids=IDS)
def test_exact_stage_behind_the_prefilters(gpu, orc, name, d, route):
    key = (name, d, cc.NR_WIDE, 0, False)
    opts = PREFILTER_ROUTES[route]
    st = all_searches(opts, key, topk_only="defer" in route)
    # the thresholded searches went through a pre-filter kernel, and their hits through the exact stage
    assert st["f16_launches"] + st["i8_launches"] > 0 and st["rescore_launches"] > 0 and st["candidates"] > 0, st
    if opts["i8"] == 0:
        assert st["i8_launches"] == 0, st
    for knn in st["knn"]:       # the k-NN went the same way: threshold passes on the pre-filter, then the exact stage
        assert knn["f16_launches"] + knn["i8_launches"] > 0 and knn["rescore_launches"] > 0 and knn["candidates"] > 0, knn
        assert opts["i8"] or knn["i8_launches"] == 0, knn
    # Deferral needs a finite error bound for the pair's panel.  Rows that fp16 cannot hold (2^100, 2^63, 2^20) or that
    # vanish in it (2^-41 and below) leave none, so of these classes only `mixed_tile` can defer, and only on the int8
    # route, whose bound is per 128-row panel of sorted rows (the fp16 panels all hold a row with an infinite norm bound).
    if name == "mixed_tile" and opts["i8"] and "defer" in route:
        assert st["deferred"] > 0, st


# Deferred variant of the exact stage with pairs really deferred on every route: `mixed_tile` in fp16's range
# (tests/chain_cases.py fp16_cases: cancelling rows in every other query row and every third reference row, all of them
# rows the fp16 and int8 images hold), on a Flat index.  (The cancelling rows alone defer nothing: their error bound is many
# times their scores.)
@pytest.mark.parametrize("route", [r for r in PREFILTER_ROUTES if "defer" in r])
@pytest.mark.parametrize("d", cc.DIMS)
def test_deferred_exact_stage_on_rows_in_fp16_range(gpu, orc, d, route):
    st = all_searches(PREFILTER_ROUTES[route], ("mixed_tile", d, cc.NR_WIDE, 0, True), topk_only=True)
    assert st["deferred"] > 0 and st["rescore_launches"] > 0, st
    assert (st["i8_launches"] > 0) if PREFILTER_ROUTES[route]["i8"] else (st["f16_launches"] > 0 and st["i8_launches"] == 0), st


# ---------------------------------------------------------------- generic score matrix
# (`sub_in` under L2: next to a query element of 2^100 a subnormal reference element lies below half an ulp of the
# difference and every distance overflows to +inf: the case pins `q - r` and the all-inf results -- no hit, every k-NN slot
# empty -- not the operands' low bits)
@pytest.mark.parametrize("name,d", CASES, ids=IDS)
def test_generic_score_matrix_l2(gpu, orc, name, d):
    """`overflow` at half the scale: `(q - r)^2` of two elements of opposite sign is finite, the second one overflows"""
    key = (name, d, cc.NR, 1, False)
    if name == "overflow":
        s = want("scores", *key)
        assert 0.05 < np.mean(s == np.inf) < 0.99 and 0.02 < np.mean(np.isfinite(s)) and not np.isnan(s).any()
    all_searches({}, key)


@pytest.mark.parametrize("name,d", CASES, ids=IDS)
def test_generic_score_matrix_k70(gpu, orc, name, d):
    check_knn(EXACT, (name, d, cc.NR, 0, False), 70)


# ---------------------------------------------------------------- SQfp16
HALF_CASES = [(name, d) for name in ("cancel", "mixed_tile", "underflow_zero") for d in cc.DIMS]


@pytest.mark.parametrize("options", [EXACT, PREFILTER_ROUTES["f16"], PREFILTER_ROUTES["i8"]], ids=["exact", "f16", "i8"])
@pytest.mark.parametrize("name,d", HALF_CASES, ids=[f"{n}-{d}" for n, d in HALF_CASES])
def test_sqfp16_index(gpu, orc, name, d, options):
    """FlatIndex(codec="SQfp16") on rows that are already half-representable (dec(r) == r): the oracle on the same rows"""
    key = (name, d, cc.NR, 0, True)
    q, r, _, _ = rows(*key)
    assert np.array_equal(dec(r), r)
    if name == "underflow_zero":
        tiny = r[0::3]
        assert (np.abs(tiny) < 2.0 ** -14).all() and (tiny != 0).all()         # subnormal in fp16
    all_searches(options, key, codec="SQfp16")
    check_knn(options, key, 70, codec="SQfp16")


def videos(x, lens, prefix):
    from vsc2022_amd.vsc.index import VideoFeature

    off = np.r_[0, np.cumsum(lens)]
    assert off[-1] <= len(x)
    return [VideoFeature(video_id=f"{prefix}{v}", feature=np.array(x[off[v]:off[v + 1]]),
                         timestamps=np.stack([np.arange(n, dtype=np.float32), np.arange(1, n + 1, dtype=np.float32)], axis=1))
            for v, n in enumerate(lens)]


@pytest.mark.parametrize("name,d", HALF_CASES, ids=[f"{n}-{d}" for n, d in HALF_CASES])
def test_sqfp16_video_index(gpu, orc, name, d):
    from vsc2022_amd.vsc.index import VideoIndex

    q, r, _, _ = rows(name, d, cc.NR, 0, True)
    vi = VideoIndex(d, "SQfp16")
    vi.add(videos(r, (40, 33, 65, 100, 62), "R"))
    K = q.shape[0] * r.shape[0] // 10
    hits = vi.search_hits(videos(q, (70, 60), "Q"), K)
    oi, oj, os_ = orc.global_threshold_search(q, r, K)
    assert np.array_equal(hits.i, oi) and np.array_equal(hits.j, oj) and np.array_equal(bits(hits.s), bits(os_))


# ---------------------------------------------------------------- Temporal Network / aligner tile
Q_LENS, R_LENS = (40, 33), (70, 65)
TN_KW = dict(tn_max_step=5, min_length=4)


def tn_inputs(name, d, half):
    if half:
        q, r = cc.fp16_cases(d, 73, 135)[name]
        return q, dec(r)
    return cc.make(name, d, 73, 135)


def check_tile(orc, name, d, half):
    from vsc2022_amd.vcsl.vta import build_vta_model
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim
    from vsc2022_amd.vsc.metrics import CandidatePair

    q, r = tn_inputs(name, d, half)
    qv, rv = videos(q, Q_LENS, "Q"), videos(r, R_LENS, "R")
    q_off, r_off = np.r_[0, np.cumsum(Q_LENS)], np.r_[0, np.cumsum(R_LENS)]
    for bias in (0.0, 0.5):
        loc = VCSLLocalizationMaxSim(qv, rv, "TN", similarity_bias=bias, ref_codec="SQfp16" if half else "Flat", **TN_KW)
        mats = []
        for p in range(2):
            sims = loc.similarity(CandidatePair(f"Q{p}", f"R{p}", 1.0))
            exp = orc.pair_sims(q[q_off[p]:q_off[p + 1]], r[r_off[p]:r_off[p + 1]], bias)
            nan = np.isnan(exp)
            assert np.array_equal(np.isnan(sims), nan), (name, d, bias, p)
            assert np.array_equal(bits(sims)[~nan], bits(exp)[~nan]), (name, d, bias, p, int((bits(sims) != bits(exp))[~nan].sum()))
            mats.append((f"{name}{p}", exp))
        # the aligners behind the tile, on the matrices without NaN (the order over NaN is undefined): TN against the
        # oracle's, the device DTW / DP against the host functions where the matrix is finite
        clean = [(label, np.ascontiguousarray(m[:, ~np.isnan(m).any(axis=0)])) for label, m in mats]
        got = build_vta_model("TN", **TN_KW).forward_sim(clean)
        for (label, m), (_, boxes) in zip(clean, got):
            assert [list(b) for b in boxes] == orc.tn(m, **TN_KW), (name, d, bias, label)
        finite = [(label, m) for label, m in clean if np.isfinite(m).all()]
        for model in ("DTW", "DP"):
            kw = dict(discontinue=3, min_sim=0.2, min_length=4, max_iou=0.3)
            if finite:
                dev = build_vta_model(model, on_device=True, **kw)
                assert dev.forward_sim(finite) == build_vta_model(model, **kw).forward_sim(finite), (name, d, bias, model)
                assert not dev.last_status.any()


@pytest.mark.parametrize("name,d", CASES, ids=IDS)
def test_tn_tile_flat(gpu, orc, name, d):
    check_tile(orc, name, d, False)


@pytest.mark.parametrize("name,d", HALF_CASES, ids=[f"{n}-{d}" for n, d in HALF_CASES])
def test_tn_tile_sqfp16(gpu, orc, name, d):
    check_tile(orc, name, d, True)


# ---------------------------------------------------------------- vsc_row_normalize
@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("d", [7, 64, 511])
def test_row_normalize(gpu, orc, n, d):
    from vsc2022_amd.vsc.baseline.score_normalization import normalize

    x = cc.normalize_rows(n, d)
    sq = x.astype(np.float64) ** 2
    if n >= 6:
        assert (sq[1] < 2.0 ** -150).all() and (x[1] != 0).all() and sq[2].sum() > 2.0 ** 128 and not x[3].any()
    with np.errstate(all="ignore"):
        exp = orc.row_normalize(x)
    got = normalize(x)
    assert not np.isnan(exp).any()
    assert np.array_equal(bits(got), bits(exp)), (n, d, np.nonzero((bits(got) != bits(exp)).any(axis=1))[0][:10])


# ---------------------------------------------------------------- the hit sort on its own
def test_sort_hits_ties_signed_zeros(gpu):
    """vsc_sort_hits orders +0.0 and -0.0 as one score, by (row, reference), and returns their bits -- with row bounds
    and without (no bound: the sort must still leave alone the key bit that carries the sign)"""
    from vsc2022_amd import _lib

    rng = np.random.default_rng(63)
    n, nrow, nref = 5000, 300, 700
    i = rng.integers(0, nrow, n).astype(np.int32)
    j = rng.integers(0, nref, n).astype(np.int32)
    s = rng.choice(np.float32([-1.5, -0.0, 0.0, 2.0 ** -149, -2.0 ** -149, np.inf, -np.inf]), n)
    order = np.lexsort((j, i, -s.astype(np.float64)))        # (float comparison: the zeros tie)
    assert (bits(s[order])[1:] != bits(s[order])[:-1])[s[order][1:] == 0].sum() > 100      # the zeros' signs interleave
    for bounds in ((nrow, nref), (0, 0)):
        oi, oj, os_ = np.empty_like(i), np.empty_like(j), np.empty_like(s)
        _lib.check(_lib.lib().vsc_sort_hits(i.ctypes.data, j.ctypes.data, s.ctypes.data, n, _lib.MEM_HOST, bounds[0], bounds[1],
                                            oi.ctypes.data, oj.ctypes.data, os_.ctypes.data, _lib.MEM_HOST, 0))
        assert np.array_equal(oi, i[order]) and np.array_equal(oj, j[order]), bounds
        assert np.array_equal(bits(os_), bits(s[order])), bounds
