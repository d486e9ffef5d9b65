"""GPU: one handle, many calls.  Every other file builds a fresh index per case; bench.py and any service keep one
handle for every step.  `DevBuf::reserve` only grows and is poisoned (VSC_POISON_ALLOC) only when it allocates, so after
a large call a smaller one runs in buffers full of plausible stale rows, thresholds, candidates and counters, and a
handle carries host state of its own (the int8 image's lazy upkeep, the excluded coordinates, the centre decided once,
the hit capacity learned from an overflow, options).  Here every step on a reused handle is compared with the CPU oracle
on the rows present (an SQfp16 index: on the rows it decodes to), the restatements of tests/, or a fresh handle given
the same inputs.  Every comparison is exact: integers and fp32 bit patterns.

L1 growth with a search after every add        L5 one DeviceMatcher, several query sets
L2 shrinking and growing workloads             L6 one DeviceScoreNormalizer
L3 searches after a kept-hit overflow          L7 the handle-less entry points' shared workspace
L4 options changed on a populated handle

tests/test_gpu_smoke.py runs this file again with poisoned allocations."""
import ctypes
import functools

import numpy as np
import pytest

from codec_rows import dec
from helpers import bits, check_localisation_sample

pytestmark = pytest.mark.gpu

D, NQ = 64, 130   # 130 query rows: one full 128-row panel plus two
COUNTS = (1, 63, 64, 65, 512, 513, 1023, 1024, 1025, 1537, 3071)   # cumulative rows after every add of L1
ROUTES = {"exact": dict(prefilter=0), "f16-panel": dict(prefilter=2, i8=0), "f16-ring": dict(prefilter=2, i8=0, f16_kernel=1),
          "int8": dict(prefilter=2, i8=2)}
CODECS = ("Flat", "SQfp16")


def _unit(rng, n, d, shift=0.5):
    """unit rows around a common offset: the mean carries ~20 % of the rows' energy, so that an int8 image that decides
    by itself (i8_center = 1, threshold 2 %) does centre"""
    x = rng.standard_normal((n, d)).astype(np.float32) + np.float32(shift)
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))


@functools.lru_cache(maxsize=None)
def rows():
    """(1100 query rows, 3071 reference rows), built once and never modified.  The reference row on each side of every
    add boundary of L1 is the same row, and a query row equals it: the best scores tie across adds.  The first NQ query
    rows are the query set of L1 and L4; rows 127 / 128 (the panel's edge) are equal."""
    rng = np.random.default_rng(2024)
    q, r = _unit(rng, 1100, D), _unit(rng, COUNTS[-1], D)
    # every second query row lies on the other side of the references' mean: an int8 row that is centred (or not) against
    # what the kernel assumes then scores too LOW in the pre-filter and loses true hits, instead of passing too many pairs
    q[1::2] = _unit(rng, 1100, D, -0.5)[1::2]
    for b in COUNTS[:-1]:
        r[b] = r[b - 1]
    for k, b in enumerate(COUNTS[:-1]):
        q[3 * k] = r[b]
    q[128] = q[127]
    q.setflags(write=False)
    r.setflags(write=False)
    return q, r


def present(r, codec):
    """the rows a search sees"""
    return r if codec == "Flat" else dec(r)


def make(codec, opts, d=D):
    from vsc2022_amd.vsc.index import FlatIndex

    return FlatIndex(d, 0, 0, options={k: float(v) for k, v in opts.items()}, codec=codec)


def same_hits(got, want, what):
    assert len(got[2]) == len(want[2]), (what, len(got[2]), len(want[2]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    assert np.array_equal(bits(got[2]), bits(want[2])), what


def check_topk(orc, idx, q, r, K, what, want=None):
    i, j, s, radius = idx.global_topk(q, K)
    oi, oj, os_, info = orc.global_threshold_search(q, r, K, 0, return_info=True) if want is None else want
    same_hits((i, j, s), (oi, oj, os_), what)
    # (the proven top-K route returns the steady run's radius, not the schedule's: tests/test_gpu_topk_proven.py)
    assert idx.get_option("last_topk_route") == 1 or bits(radius) == bits(info["radius"]), (what, radius, info)
    return info


def check_knn(orc, idx, q, r, k, what, want=None):
    Dk, I = idx.search(q, k)
    oD, oI = orc.knn(q, r, k) if want is None else want
    assert np.array_equal(I, oI), what
    assert np.array_equal(bits(Dk), bits(oD)), what


def check_range(orc, idx, q, r, radius, what, want=None):
    lims, Dr, I = idx.range_search(q, radius)
    ol, oD, oI = orc.range_search(q, r, radius) if want is None else want
    assert np.array_equal(lims, ol) and np.array_equal(I, oI) and np.array_equal(bits(Dr), bits(oD)), what
    return lims


# ---------------------------------------------------------------------------------- L1: growth, a search after every add

@functools.lru_cache(maxsize=None)
def l1_reference(codec, n):
    import oracle as orc

    q, r = rows()
    q, r = q[:NQ], present(r[:n], codec)
    return {"topk": {K: orc.global_threshold_search(q, r, K, 0, return_info=True) for K in (1, 300, 10 ** 6)},
            "knn": {k: orc.knn(q, r, k) for k in {1, min(5, n)}}, "range": orc.range_search(q, r, 0.1)}


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("route", list(ROUTES) + ["int8-centre-1", "int8-centre-2"])
def test_l1_growth_with_a_search_after_every_add(gpu, orc, route, codec):
    """Adds that cross the 64-row fragment tiles, the 512-row padding of the images, the 1024-row centre decision and
    several reallocations (with copies) of the images; after each: top-K at K = 1, 300 and more than the matrix, k-NN,
    a range search.  The int8 route also with the centre left to the data (decided once, at 1024 rows) and forced."""
    opts = dict(ROUTES["int8"], i8_center=int(route[-1])) if route.startswith("int8-centre") else ROUTES[route]
    q, r = rows()
    q = q[:NQ]
    idx = make(codec, opts)
    idx.profile(True)
    sizes, n0 = [idx.get_option("ref_bytes")], 0
    for n in COUNTS:
        idx.add(r[n0:n])
        n0 = n
        assert idx.ntotal == n
        sizes.append(idx.get_option("ref_bytes"))
        seen, want = present(r[:n], codec), l1_reference(codec, n)
        for K, w in want["topk"].items():
            check_topk(orc, idx, q, seen, K, (route, codec, n, "top-K", K), w)
        for k, w in want["knn"].items():
            check_knn(orc, idx, q, seen, k, (route, codec, n, "k-NN", k), w)
        check_range(orc, idx, q, seen, 0.1, (route, codec, n, "range"), want["range"])
    assert sum(b > a for a, b in zip(sizes[:-1], sizes[1:])) >= 3, sizes
    if route.startswith("int8-centre"):
        assert idx.get_option("i8_center_on") == 1, idx.get_option("i8_center_share")
    st = idx.profile_read()   # the route's own kernels ran
    if route.startswith("int8"):
        assert st["i8_launches"] > 0 and st["rescore_launches"] > 0 and idx.get_option("i8_fallbacks") == 0, st
    elif route.startswith("f16"):
        assert st["f16_launches"] > 0 and st["rescore_launches"] > 0 and st["i8_launches"] == 0, st
    else:
        assert st["sim_launches"] > 0 and st["f16_launches"] == 0 and st["i8_launches"] == 0, st


# ---------------------------------------------------------------------------------- L2: shrinking and growing workloads

L2_STEPS = (("topk", 1100, 300000), ("topk", 1, 1), ("topk", 129, 50), ("knn", 1100, 64), ("knn", 3, 1), ("range", 700, "median"),
            ("range", 2, 10.0), ("topk", NQ, 10 ** 6), ("topk", 33, 7))
L2_REFS, L2_CAP = 3000, 400000


@functools.lru_cache(maxsize=None)
def l2_reference(codec, step):
    """(oracle result, entries the kept-hit buffer must hold) of one step of L2"""
    import oracle as orc

    kind, nq, arg = L2_STEPS[step]
    q, r = rows()
    q, r = q[:nq], present(r[:L2_REFS], codec)
    S = orc.scores(q, r)
    if kind == "knn":
        return orc.knn(q, r, arg), 0, arg
    if kind == "range":
        radius = float(np.median(S)) if arg == "median" else arg
        res = orc.range_search(q, r, radius)
        return res, len(res[1]), radius
    # The longest kept list: the reference's schedule replayed on the oracle's scores.  The product defines that schedule
    # in one place, the batch loop of global_topk_impl (vsc2022_amd/csrc/api_search.hip: `bs = 32`, `if (bs < 20000) bs *= 2`,
    # the re-threshold at kept > 2K), and the oracle in orc_global_threshold_search (oracle/vsc_oracle.c), which reports its
    # radius and event count only -- hence the copy here; a change of either has to be made in this loop too.  It cannot
    # drift unseen: the steps of this test that must overflow and the ones that must not are decided by it.
    radius, kept, need, bs, i0 = np.float32(-1e10), np.empty(0, np.float32), 0, 32, 0
    while i0 < nq:
        new = S[i0:i0 + bs].ravel()
        kept = np.concatenate([kept, new[new > radius]])
        need = max(need, len(kept))
        if len(kept) > 2 * arg:
            radius = np.sort(kept)[::-1][arg]
            kept = kept[kept > radius]
        i0 += bs
        if bs < 20000:
            bs *= 2
    return orc.global_threshold_search(q, r, arg, 0, return_info=True), need, arg


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_l2_shrinking_and_growing_workloads(gpu, orc, route, codec):
    """Nine calls of very different sizes on 3000 fixed references, in order and then reversed: a small call runs in the
    buffers a large one left behind.  The same on a second handle whose kept-hit buffer the caller sized once (400 000
    entries): a step whose hits do not fit it -- by the schedule replayed on the oracle's scores, or the oracle's count of
    range hits -- must fail with VSC_ERR_OVERFLOW as include/vscmi.h says, every other step must equal the oracle, the
    ones after a failed call included.  (A k-NN whose pre-filtered pass overflows falls back to the exact kernel.)"""
    from vsc2022_amd import _lib

    q, r = rows()
    seen = present(r[:L2_REFS], codec)
    order = list(range(len(L2_STEPS))) + list(range(len(L2_STEPS)))[::-1]
    for cap in (0, L2_CAP):
        idx = make(codec, ROUTES[route])
        idx.add(r[:L2_REFS])
        if cap:
            idx.set_hit_capacity(cap)
        failed = 0
        for pos, step in enumerate(order):
            kind, nq, _ = L2_STEPS[step]
            want, need, arg = l2_reference(codec, step)
            what = (route, codec, cap, pos, L2_STEPS[step])
            call = {"topk": check_topk, "knn": check_knn, "range": check_range}[kind]
            if cap and need > cap:
                with pytest.raises(_lib.VscError) as e:
                    call(orc, idx, q[:nq], seen, arg, what, want)
                assert e.value.code == _lib.VSC_ERR_OVERFLOW, what
                failed += 1
                continue
            out = call(orc, idx, q[:nq], seen, arg, what, want)
            if kind == "range" and arg == 10.0:
                assert not out.any(), what   # no hit: lims all zero
        assert failed == (4 if cap else 0)   # (K = 300 000 and the median range search, both ways)


# ---------------------------------------------------------------------------------- L3: after an overflow

@functools.lru_cache(maxsize=None)
def l3_rows():
    """the inputs of test_gpu_smoke.py::test_overflow_retry_in_fresh_process, and 100 more reference rows"""
    rng = np.random.default_rng(5)
    r = rng.standard_normal((900, 64)).astype(np.float32)
    q = rng.standard_normal((300, 64)).astype(np.float32)
    r = np.concatenate([r, rng.standard_normal((100, 64)).astype(np.float32)])
    r[900], r[901] = r[899], r[17]   # ties that straddle the add
    q.setflags(write=False)
    r.setflags(write=False)
    return q, r


@functools.lru_cache(maxsize=None)
def l3_reference(n, K):
    import oracle as orc

    q, r = l3_rows()
    return orc.global_threshold_search(q, r[:n], K, 0, return_info=True)


@pytest.mark.parametrize("defer", [0, 1, 2])
@pytest.mark.parametrize("route", ["f16-panel", "int8"])
def test_l3_searches_after_an_overflow(gpu, orc, route, defer):
    """K = 14 400 over 900 references: the default kept-hit buffer holds 32 x 900 + 2K + 2K + 1024 = 58 624 entries, the
    second batch keeps 96 x 900 = 86 400, the search is rerun and the handle remembers the capacity it ended with.  Then
    a small top-K, a k-NN, a range search, an add and the large search again on that handle."""
    q, r = l3_rows()
    K = 14400
    idx = make("Flat", dict(ROUTES[route], defer=defer))
    idx.add(r[:900])
    assert idx.get_option("hit_cap_learned") == 0
    check_topk(orc, idx, q, r[:900], K, (route, defer, "the search that overflows"), l3_reference(900, K))
    # It did overflow, once: the handle starts its next searches at four times the default buffer.  Without deferral that
    # follows from the scores alone.  With it the second batch may leave most of its pairs in the deferred set, which is
    # not part of the kept list (the int8 route with defer = 1 does, and never overflows): such a handle repeats the
    # search with deferral off, so that every case goes on from a handle that was rerun.
    learned = 4 * (max(32 * 900, 2 * K) + 2 * K + 1024)
    if defer and idx.get_option("hit_cap_learned") == 0:
        idx.set_option("defer", 0)
        check_topk(orc, idx, q, r[:900], K, (route, defer, "the search that overflows, deferral off"), l3_reference(900, K))
        idx.set_option("defer", defer)
    assert idx.get_option("hit_cap_learned") == learned == 234496, (route, defer, idx.get_option("hit_cap_learned"))
    check_topk(orc, idx, q, r[:900], 100, (route, defer, "K = 100"), l3_reference(900, 100))
    # three query rows: the whole matrix (3 x 900 + 1024 entries) is smaller than the capacity the handle learned
    check_topk(orc, idx, q[:3], r[:900], 100, (route, defer, "K = 100, 3 rows"))
    check_knn(orc, idx, q, r[:900], 8, (route, defer, "8-NN"))
    lims = check_range(orc, idx, q, r[:900], 20.0, (route, defer, "range"))
    assert 100 < lims[-1] < 20000
    idx.add(r[900:])
    info = check_topk(orc, idx, q, r, K, (route, defer, "after the add"), l3_reference(1000, K))
    fresh = make("Flat", dict(ROUTES[route], defer=defer))
    fresh.add(r)
    check_topk(orc, fresh, q, r, K, (route, defer, "fresh handle"), l3_reference(1000, K))
    # (over 1000 rows the first batch's 32 000 scores exceed 2K and are cut to K at once: nothing overflows any more, the
    # reused handle keeps what it learned and the fresh one learns nothing)
    assert idx.get_option("hit_cap_learned") == learned and fresh.get_option("hit_cap_learned") == 0
    for name in ("n_rethreshold", "deferred"):
        assert idx.get_option(name) == fresh.get_option(name), (route, defer, name)
    assert idx.get_option("n_rethreshold") == info["n_rethreshold"]
    if defer != 1:   # (1 defers where it expects an event to follow; 2 every pre-filtered batch)
        assert (fresh.get_option("deferred") > 0) == (defer == 2), (route, defer, fresh.get_option("deferred"))


# ---------------------------------------------------------------------------------- L4: options on a populated handle

L4_WALK = (("prefilter", 1), ("prefilter", 2), ("i8", 1), ("i8", 2), ("defer", 0), ("defer", 1), ("defer", 2), ("defer_i8", 0),
           ("defer_i8", 1), ("i8_screen", 1), ("i8_screen", 0), ("i8p_pair", 0), ("i8p_pair", 1), ("i8p_pair", 2), ("i8_sort", 0),
           ("i8_sort", 1), ("i8_group", 0), ("i8_group", 7), ("i8_group", 12), ("rescore_sort", 0), ("rescore_sort", 1),
           ("topk_shortcut", 0), ("topk_shortcut", 2), ("knn_levels", 1), ("knn_levels", 0), ("knn_first_tile", 0),
           ("knn_first_tile", 1), ("knn_nchunk", 1), ("knn_nchunk", 3), ("knn_nchunk", 64), ("knn_ratio", 3), ("knn_step", 32768),
           ("density_hint", 0), ("density_hint", 1), ("density_hint", 1e-3), ("density_hint", 1e-9), ("sort_hits", 0),
           ("sort_hits", 1))
L4_REFS, L4_K = 1537, 900


@functools.lru_cache(maxsize=None)
def l4_reference(codec):
    import oracle as orc

    q, r = rows()
    q, r = q[:NQ], present(r[:L4_REFS], codec)
    return orc.global_threshold_search(q, r, L4_K, 0, return_info=True), orc.knn(q, r, 5), orc.scores(q, r)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_l4_options_changed_on_a_populated_handle(gpu, orc, route, codec):
    """Every option that may change once rows exist, one after the other and then backwards, a top-K and a 5-NN after
    each change.  A change that would need an image of the rows the handle never kept must be refused and change
    nothing; so must the options that decide which images exist."""
    q, r = rows()
    q, seen = q[:NQ], present(r[:L4_REFS], codec)
    want_topk, want_knn, S = l4_reference(codec)
    opts = ROUTES[route]
    idx = make(codec, opts)
    idx.add(r[:1000])
    idx.add(r[1000:L4_REFS])
    back = L4_WALK[-2:] + L4_WALK[-3::-1]   # (backwards, but the unsorted result is switched off again before the rest)
    for pos, (name, value) in enumerate(L4_WALK + back):
        what = (route, codec, pos, name, value)
        no_image = (name == "prefilter" and opts["prefilter"] == 0) or (name == "i8" and opts.get("i8", 0) == 0 and opts["prefilter"] != 0)
        if no_image:
            before = idx.get_option(name)
            with pytest.raises(ValueError):
                idx.set_option(name, value)
            assert idx.get_option(name) == before, what
        else:
            idx.set_option(name, value)
        if idx.get_option("sort_hits") == 0:
            # the kept hits as they lie (tests/test_gpu_options.py, test_unsorted_hits_are_the_same_set): K of more than K
            # kept hits are pairs of the matrix beyond the radius; a search nothing is cut from returns the whole set
            ui, uj, us, urad = idx.global_topk(q, L4_K)
            assert len(us) == L4_K and len(set(zip(ui.tolist(), uj.tolist()))) == L4_K, what
            assert np.array_equal(bits(us), bits(S[ui, uj])) and (us > np.float32(urad)).all(), what
            assert idx.get_option("last_topk_route") == 1 or bits(urad) == bits(want_topk[3]["radius"]), what
            ui, uj, us, _ = idx.global_topk(q, 10 ** 6)
            order = np.lexsort((uj, ui))
            assert len(us) == S.size and np.array_equal(ui[order], np.repeat(np.arange(NQ), L4_REFS)), what
            assert np.array_equal(uj[order], np.tile(np.arange(L4_REFS), NQ)) and np.array_equal(bits(us[order]), bits(S.ravel())), what
        else:
            check_topk(orc, idx, q, seen, L4_K, what, want_topk)
        check_knn(orc, idx, q, seen, 5, what, want_knn)
    # decided while the handle is empty: refused now, whatever the route
    for name, value in (("prefilter", 0 if opts["prefilter"] else 2), ("f16_kernel", 1 - idx.get_option("f16_kernel")),
                        ("i8_exclude", 1 - idx.get_option("i8_exclude")), ("i8_center", (idx.get_option("i8_center") + 1) % 3)):
        before = idx.get_option(name)
        with pytest.raises(ValueError):
            idx.set_option(name, value)
        assert idx.get_option(name) == before, (route, codec, name)
    if opts.get("i8", 0):
        with pytest.raises(ValueError):
            idx.set_option("i8", 0)
    check_topk(orc, idx, q, seen, L4_K, (route, codec, "after the refusals"), want_topk)


# ---------------------------------------------------------------------------------- L5: one DeviceMatcher, several query sets

TN_HBM = dict(tn_top_k=16, tn_max_step=64)   # more DP state than LDS holds: the kernel keeps it in HBM


@functools.lru_cache(maxsize=None)
def l5_sets():
    """references: 60 videos of 8-80 frames; query sets A (40 videos of 8-60 frames), B (3 videos of 1, 2 and 5 frames) and
    C (120 videos of 8-60 frames).  Every second query video is a noised copy of a stretch of a reference video.
    -> ({name: (rows, offsets, timestamps)}, the same for the references)"""
    rng = np.random.default_rng(55)

    def pack(vids):
        off = np.r_[0, np.cumsum([len(v) for v in vids])].astype(np.int64)
        feats = np.ascontiguousarray(np.concatenate(vids), dtype=np.float32)
        t = np.concatenate([np.arange(len(v), dtype=np.float32) for v in vids])
        feats.setflags(write=False)
        return feats, off, np.ascontiguousarray(np.stack([t, t + 1], axis=1))

    refs = [_unit(rng, int(n), D, 0.0) for n in rng.integers(8, 81, 60)]

    def queries(lens):
        out = []
        for k, n in enumerate(lens):
            v = _unit(rng, int(n), D, 0.0)
            if k % 2 == 0:
                src = refs[int(rng.integers(0, len(refs)))]
                m = min(int(n), len(src))
                a = int(rng.integers(0, len(src) - m + 1))
                x = src[a:a + m] + np.float32(0.05) * rng.standard_normal((m, D)).astype(np.float32)
                v[:m] = x / np.linalg.norm(x, axis=1, keepdims=True)
            out.append(v)
        return out

    sets = {"A": pack(queries(rng.integers(8, 61, 40))), "B": pack(queries([1, 2, 5])), "C": pack(queries(rng.integers(8, 61, 120)))}
    return sets, pack(refs)


def _l5_matcher(tn_codec):
    from vsc2022_amd.engine import DeviceMatcher

    rf, roff, rts = l5_sets()[1]
    return DeviceMatcher(rf, roff, 0, tn_codec=tn_codec, r_ts=rts)


def _l5_run(m, name):
    """Every call of L5 on the query set `name`; each result is copied before the next call (results are views of buffers
    the matcher reuses).  -> {what: numpy arrays}"""
    import torch

    qf, qoff, qts = l5_sets()[0][name]
    m.set_queries(qf, qoff, q_ts=qts)
    out = {}

    def boxes_of(nbox, boxes, score):
        nbox, boxes, score = (t.cpu().numpy().copy() for t in (nbox, boxes, score))
        valid = np.arange(boxes.shape[1])[None, :] < nbox[:, None]   # (slots beyond nbox are not part of a result)
        return {"nbox": nbox, "boxes": boxes[valid], "box_score": bits(score[valid])}

    def result(res):
        d = {"counts": np.array([res.n_hits, res.n_pairs, res.n_candidates, res.n_localized, res.n_matches]),
             "radius": bits(res.radius), "cand_q": res.cand_q.cpu().numpy().copy(), "cand_r": res.cand_r.cpu().numpy().copy(),
             "cand_score": bits(res.cand_score.cpu().numpy()), "loc_index": res.loc_index.cpu().numpy().copy()}
        d.update(boxes_of(res.nbox, res.boxes, res.box_score))
        if res.row_cand is not None:
            for f in ("row_cand", "row_q", "row_r", "row_times", "row_boxes"):
                d[f] = getattr(res, f).cpu().numpy().copy()
            d["row_score"] = bits(res.row_score.cpu().numpy())
        return d

    out["match"] = result(m.match())
    out["rows"] = result(m.match(rows=True))
    out["sum"] = result(m.match(aggregation="sum"))
    n_loc = int(out["match"]["counts"][3])
    pq = torch.from_numpy(out["match"]["cand_q"][:n_loc]).to(m.tdev)
    pr = torch.from_numpy(out["match"]["cand_r"][:n_loc]).to(m.tdev)
    for what, kw in (("tn", {}), ("tn_hbm", TN_HBM), ("tn_again", {})):
        nbox, boxes, score = m.localize(pq, pr, 0.0, **kw)
        out[what] = dict(boxes_of(nbox, boxes, score), all_boxes=boxes.cpu().numpy().copy(), all_score=score.cpu().numpy().copy())
    return out


@functools.lru_cache(maxsize=None)
def l5_fresh(tn_codec, name):
    """what a matcher built for this query set alone returns"""
    return _l5_run(_l5_matcher(tn_codec), name)


@pytest.mark.parametrize("tn_codec", CODECS)
def test_l5_one_matcher_several_query_sets(gpu, orc, tn_codec):
    """A (40 videos), B (8 rows in all), C (120 videos), A again through `set_queries` on one matcher: the Temporal-Network context
    repacks only the query side, the search, candidate and box buffers are reused.  match(), match(rows=True),
    match(aggregation="sum") and the localisation with the state in LDS, in HBM and in LDS again equal what a fresh matcher
    returns; a sample of 50 pairs ties boxes and MaxSim bits to the oracle."""
    import torch

    sets, (rf, roff, _) = l5_sets()
    m = _l5_matcher(tn_codec)
    r_seen = torch.from_numpy(present(rf, tn_codec))   # (tn_codec: the aligner sees the rows rounded to half floats)
    for pos, name in enumerate("ABCA"):
        got, want = _l5_run(m, name), l5_fresh(tn_codec, name)
        assert got.keys() == want.keys()
        for call in want:
            for f in want[call]:
                if not f.startswith("all_"):
                    assert np.array_equal(got[call][f], want[call][f]), (tn_codec, pos, name, call, f)
        for f in ("nbox", "boxes", "box_score"):
            assert np.array_equal(got["tn"][f], got["tn_again"][f]) and np.array_equal(got["tn"][f], got["match"][f]), (pos, name, f)
        if name != "B":   # (B's videos of 1, 2 and 5 frames need not hold a box)
            assert got["match"]["counts"][4] > 0 and got["tn_hbm"]["nbox"].sum() > 0
        qf, qoff, _ = sets[name]
        n_loc = int(got["match"]["counts"][3])
        pq, pr = got["match"]["cand_q"][:n_loc], got["match"]["cand_r"][:n_loc]
        for call, kw in (("tn", dict(tn_max_step=5, min_length=4)), ("tn_hbm", TN_HBM)):
            n, _ = check_localisation_sample(orc, torch.from_numpy(qf), qoff, r_seen, roff, pq, pr, got[call]["nbox"], got[call]["all_boxes"],
                                             got[call]["all_score"], 0.0, n=50, seed=pos, tn_kw=kw)
            assert n == min(50, n_loc)


# ---------------------------------------------------------------------------------- L6: one DeviceScoreNormalizer

def test_l6_one_score_normalizer_many_batches(gpu):
    import torch

    from vsc2022_amd.engine import DeviceScoreNormalizer, score_normalize_device

    rng = np.random.default_rng(66)
    dev = torch.device("cuda", 0)
    draw = lambda n: torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32) * np.linspace(0.1, 1.0, D, dtype=np.float32)).to(dev)
    noise = draw(1500)
    noise[7] = 0.0   # (a zero row stays zero)
    norm = DeviceScoreNormalizer(noise, beta=1.2)
    tiny = draw(1)
    for nq, nr in ((700, 300), (1, 2), (129, 300), (700, 2)):
        q, r = draw(nq), draw(nr)
        q[nq // 2] = noise[3]   # (its best noise score ties with a noise row's own)
        got_q, got_r = norm.queries(q).clone(), norm.refs(r).clone()
        want_q, _ = score_normalize_device(q, tiny, noise, beta=1.2)
        _, want_r = score_normalize_device(tiny, r, noise, beta=1.2)
        assert got_q.shape == (nq, D) and got_r.shape == (nr, D)
        assert torch.equal(got_q.view(torch.int32), want_q.view(torch.int32)), (nq, nr)
        assert torch.equal(got_r.view(torch.int32), want_r.view(torch.int32)), (nq, nr)


# ---------------------------------------------------------------------------------- L7: the handle-less entry points

CANARY_I, CANARY_F = -77, np.float32(-7.25)


def _l7_pair_aggregate():
    from pair_agg_ref import assert_columns, case, pair_aggregate_ref
    from vsc2022_amd import _lib

    i, j, s, row2q, row2r = case("quantised")
    n = len(s)
    assert n == 20000
    exp = pair_aggregate_ref(i, j, s, row2q, row2r, "sum")
    out = [np.full(n + 3, CANARY_I, dtype=dt) for dt in (np.int32, np.int32, np.float32, np.int64, np.int32)]
    n_pairs = ctypes.c_int64(0)
    _lib.check(_lib.lib().vsc_pair_aggregate(i.ctypes.data, j.ctypes.data, s.ctypes.data, n, 0, row2q.ctypes.data, len(row2q),
                                             row2r.ctypes.data, len(row2r), 0, 1, _lib.AGG_SUM, 1, *(a.ctypes.data for a in out), n, 0,
                                             ctypes.byref(n_pairs), 0))
    k = n_pairs.value
    assert_columns(tuple(a[:k] for a in out), exp, "vsc_pair_aggregate")
    assert all((a[k:] == CANARY_I).all() for a in out), "vsc_pair_aggregate wrote beyond the pairs it reported"


def _l7_sort_hits():
    from vsc2022_amd import _lib

    i = np.array([3, 0, 3, 1, 0], dtype=np.int32)
    j = np.array([9, 2, 4, 4, 1], dtype=np.int32)
    s = np.array([0.5, -0.0, 0.5, 2.0, 0.0], dtype=np.float32)
    order = np.lexsort((j, i, -s.astype(np.float64)))
    oi, oj, os_ = np.full(8, CANARY_I, np.int32), np.full(8, CANARY_I, np.int32), np.full(8, CANARY_F, np.float32)
    _lib.check(_lib.lib().vsc_sort_hits(i.ctypes.data, j.ctypes.data, s.ctypes.data, 5, 0, 4, 10, oi.ctypes.data, oj.ctypes.data,
                                        os_.ctypes.data, 0, 0))
    assert np.array_equal(oi[:5], i[order]) and np.array_equal(oj[:5], j[order]) and np.array_equal(bits(os_[:5]), bits(s[order]))
    assert (oi[5:] == CANARY_I).all() and (oj[5:] == CANARY_I).all() and (os_[5:] == CANARY_F).all()


def _l7_pair_max():
    import oracle as orc
    from vsc2022_amd import _lib

    i, j, s = np.array([4], np.int32), np.array([7], np.int32), np.array([0.375], np.float32)
    row2q, row2r = np.repeat(np.arange(3, dtype=np.int32), 2), np.repeat(np.arange(5, dtype=np.int32), 2)
    oq, orr, os_, of = orc.pair_max(i, j, s, row2q, row2r)
    gq, gr, gs, gf = (np.full(4, CANARY_I, dtype=dt) for dt in (np.int32, np.int32, np.float32, np.int64))
    n_pairs = ctypes.c_int64(0)
    _lib.check(_lib.lib().vsc_pair_max(i.ctypes.data, j.ctypes.data, s.ctypes.data, 1, 0, row2q.ctypes.data, len(row2q), row2r.ctypes.data,
                                       len(row2r), 0, gq.ctypes.data, gr.ctypes.data, gs.ctypes.data, gf.ctypes.data, 1, 0,
                                       ctypes.byref(n_pairs), 0))
    assert n_pairs.value == 1 == len(oq)
    assert (gq[0], gr[0], gf[0]) == (oq[0], orr[0], of[0]) == (2, 3, 0) and bits(gs[:1]) == bits(os_)
    assert all((a[1:] == CANARY_I).all() for a in (gq, gr, gs, gf))


def _l7_argsort_scores():
    from vsc2022_amd import _lib

    x = np.random.default_rng(71).choice(np.array([-1.5, -0.0, 0.0, 0.25, 0.25, 3.0], dtype=np.float32), 4097)
    perm = np.full(4097 + 3, CANARY_I, np.int32)
    _lib.check(_lib.lib().vsc_argsort_scores(x.ctypes.data, 4097, 0, perm.ctypes.data, 0, 0))
    want = np.argsort(-(x.astype(np.float64) + 0.0), kind="stable")   # (-0.0 == +0.0: both negate to a zero)
    assert np.array_equal(perm[:4097], want) and (perm[4097:] == CANARY_I).all()


def _l7_filter_hits():
    import torch
    from vsc2022_amd import _lib

    rng = np.random.default_rng(72)
    n = 2049
    x = rng.standard_normal(n).astype(np.float32)
    i, j = rng.integers(0, 1 << 20, n).astype(np.int32), rng.integers(0, 1 << 21, n).astype(np.int32)
    radius = float(np.median(x))
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(a).to(dev) for a in (i, j, x)]
    outs = [torch.full((n + 3,), CANARY_I, dtype=t.dtype, device=dev) for t in ins]
    torch.cuda.synchronize(dev)
    kept = ctypes.c_int64(0)
    _lib.check(_lib.lib().vsc_filter_hits(*(t.data_ptr() for t in ins), n, radius, *(t.data_ptr() for t in outs), ctypes.byref(kept), 0))
    gi, gj, gs = (t.cpu().numpy() for t in outs)
    keep = x > np.float32(radius)
    m = kept.value
    assert m == int(keep.sum()) == 1024
    want = sorted(zip(i[keep].tolist(), j[keep].tolist(), bits(x[keep]).tolist()))
    assert sorted(zip(gi[:m].tolist(), gj[:m].tolist(), bits(gs[:m]).tolist())) == want
    assert (gi[m:] == CANARY_I).all() and (gj[m:] == CANARY_I).all() and (gs[m:] == CANARY_I).all()


def _l7_match_metric():
    import match_metric_ref as mm
    from helpers import check_match_metric_case

    n_pred, n_gt, n_pairs = mm.SHAPES[0]
    gt, pred = mm.coarse_case(0, n_pairs, n_pred, n_gt, "distinct")
    check_match_metric_case(gt, pred)   # (the restatement's group sums, match_metric's curve, canaries behind the groups)


def _l7_row_normalize():
    import oracle as orc
    from vsc2022_amd import _lib

    x = np.random.default_rng(73).standard_normal((3, 7)).astype(np.float32)
    x[1] = 0.0
    out = np.full((4, 7), CANARY_F, np.float32)
    _lib.check(_lib.lib().vsc_row_normalize(x.ctypes.data, 3, 7, 0, out.ctypes.data, 0, 0))
    assert np.array_equal(bits(out[:3]), bits(orc.row_normalize(x))) and (out[3] == CANARY_F).all()


def test_l7_handle_less_entry_points_share_one_workspace(gpu, orc):
    """vsc_pair_aggregate (20 000 hits), vsc_sort_hits (5), vsc_pair_max (1), vsc_argsort_scores (4097), vsc_filter_hits
    (2049), vsc_match_metric (one row) and vsc_row_normalize (3 x 7) run in one per-device workspace: in this order and in
    the reverse one, each against the restatement its own test file uses; outputs are pre-filled with canaries and nothing
    beyond the reported count may be written."""
    calls = (_l7_pair_aggregate, _l7_sort_hits, _l7_pair_max, _l7_argsort_scores, _l7_filter_hits, _l7_match_metric,
             _l7_row_normalize)
    for call in calls + calls[::-1]:
        call()
