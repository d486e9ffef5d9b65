"""The SQfp16 codec on the GPU: an SQfp16 index of rows X behaves, bit for bit, as the Flat index of
dec(X) = X.astype(float16).astype(float32) -- on every route of both metrics -- while it keeps the rows once, as half
floats.  Every equality is exact: rows, references, score bits, the returned radius.
"""
import ctypes

import numpy as np
import pytest

import codec_rows as cr
import prefilter_bounds as pb
from codec_rows import dec
from helpers import bits

pytestmark = pytest.mark.gpu

IP, L2 = 0, 1


def make(d, codec, options=None, metric=IP, rows=None):
    from vsc2022_amd.vsc.index import FlatIndex

    idx = FlatIndex(d, metric, 0, options={k: float(v) for k, v in (options or {}).items()}, codec=codec)
    idx.profile(True)
    if rows is not None:
        idx.add(rows)
    return idx


# ------------------------------------------------------------------------------------------------ 1. the store
@pytest.mark.parametrize("d", [16, 100, 256, 512, 768])
@pytest.mark.parametrize("ring", [0, 1])
def test_store_holds_dec_of_the_rows(gpu, d, ring):
    """Both store layouts (fragment-major for padded dims <= 512, natural above and with f16_kernel = 1), padded and
    unpadded dims; one add, many small adds that straddle the 64-row tiles, and the three kinds of source."""
    import torch

    x = cr.rows(d, 777, d)
    want = dec(x)
    opts = {"f16_kernel": ring}
    one = make(d, "SQfp16", opts, rows=x)
    assert one.codec == "SQfp16" and one.get_option("codec") == 1.0 and one.ntotal == len(x)
    assert np.array_equal(bits(one.reconstruct_n(0, len(x))), bits(want))
    assert np.array_equal(bits(one.reconstruct_n(100, 13)), bits(want[100:113]))
    many = make(d, "SQfp16", opts)
    cuts = [0, 1, 2, 63, 64, 65, 130, 190, 193, 320, 511, 513, 777]
    for a, b in zip(cuts[:-1], cuts[1:]):
        many.add(x[a:b])
    assert many.ntotal == len(x) and np.array_equal(bits(many.reconstruct_n()), bits(want))
    half = x.astype(np.float16)
    for src in (half, torch.from_numpy(half).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(half)):
        idx = make(d, "SQfp16", opts)
        idx.add(src[:300])
        idx.add(src[300:])
        assert np.array_equal(bits(idx.reconstruct_n()), bits(want))
    # a Flat index takes half rows too: the result of adding the upcast array; and reconstructs what it was given
    flat = make(d, "Flat", opts)
    flat.add(half[:70])
    flat.add(torch.from_numpy(half[70:]).cuda())
    assert flat.codec == "Flat" and flat.get_option("codec") == 0.0
    assert np.array_equal(bits(flat.reconstruct_n()), bits(want))
    flat32 = make(d, "Flat", opts, rows=x)
    assert np.array_equal(bits(flat32.reconstruct_n()), bits(x))


@pytest.mark.parametrize("d,ring", [(100, 0), (768, 0), (64, 1)])
@pytest.mark.parametrize("bad", [1e5, -7e4, np.nan, np.inf])
def test_rows_fp16_cannot_hold_fail_the_add(gpu, d, ring, bad):
    import torch

    x = cr.rows(1, 300, d)
    idx = make(d, "SQfp16", {"f16_kernel": ring}, rows=x[:150])
    y = x[150:].copy()
    y[77, d - 1] = bad
    for src in (y, torch.from_numpy(y).cuda()):
        with pytest.raises(ValueError):
            idx.add(src)
        assert idx.ntotal == 150
    if not np.isfinite(bad):
        with pytest.raises(ValueError):
            idx.add(y.astype(np.float16))
        assert idx.ntotal == 150
    # the index is as it was: the same rows, the same results, and it still grows
    assert np.array_equal(bits(idx.reconstruct_n()), bits(dec(x[:150])))
    idx.add(x[150:])
    ref = make(d, "Flat", {"f16_kernel": ring}, rows=dec(x))
    q = cr.rows(2, 40, d)
    assert np.array_equal(bits(idx.reconstruct_n()), bits(dec(x)))
    for a, b in zip(idx.global_topk(q, 500), ref.global_topk(q, 500)):
        assert np.array_equal(bits(a), bits(b)) if isinstance(a, np.ndarray) and a.dtype == np.float32 else np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 2. the routes
def shifted_rows(seed, n, d):
    x = cr.rows(seed, n, d)
    x += np.float32(0.6) * cr.unit(np.random.default_rng(99), 1, d)
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))


# route -> (handle options, dimension, kind of rows, which launches prove the route)
ROUTES = {
    "default": ({}, 64, "ties", None),
    "prefilter-off": (dict(prefilter=0), 100, "ties", "sim"),
    "f16-panel-512": (dict(prefilter=2, i8=0), 512, "ties", "f16"),
    "f16-ring-768": (dict(prefilter=2, i8=0, f16_kernel=1), 768, "ties", "f16"),
    "f16-ring-100": (dict(prefilter=2, i8=0, f16_kernel=1), 100, "ties", "f16"),
    "i8-single-128": (dict(prefilter=2, i8=2, i8p_pair=0), 128, "ties", "i8"),
    "i8-pair-256": (dict(prefilter=2, i8=2, i8p_pair=2), 256, "ties", "i8"),
    "i8-excluded-128": (dict(prefilter=2, i8=2), 128, "excluded", "i8"),
    "i8-centred-256": (dict(prefilter=2, i8=2, i8_center=2), 256, "centred", "i8"),
    "i8-screen-512": (dict(prefilter=2, i8=2, i8_screen=1), 512, "ties", "i8"),
    "segments-f16-64": (dict(prefilter=2, i8=0, rescore_sort=0), 64, "ties", "f16"),
    "segments-i8-ring-100": (dict(prefilter=2, i8=2, rescore_sort=0, f16_kernel=1), 100, "ties", "i8"),
}


def route_rows(route):
    _, d, kind, _ = ROUTES[route]
    nq, nr = 300, 2600
    if kind == "centred":
        return shifted_rows(31, nq, d), shifted_rows(32, nr, d)
    q, r = cr.with_ties(17, nq, nr, d)
    if kind == "excluded":
        r[:, 5] = np.float32(0.7001)   # (not a half: the agreement must hold on the DECODED values)
        r[:, 9] = np.float32(-1.5)
    return q, r


def candidates(idx, q, K, row2q, row2r):
    from vsc2022_amd import _lib

    q = np.ascontiguousarray(q, dtype=np.float32)
    cap = int(row2q.max() + 1) * int(row2r.max() + 1)
    oq, orr, os_ = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.float32)
    n_pairs, n_hits = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().vsc_index_candidates(idx.handle, q.ctypes.data, len(q), _lib.MEM_HOST, int(K), row2q.ctypes.data,
                                               row2r.ctypes.data, oq.ctypes.data, orr.ctypes.data, os_.ctypes.data, cap,
                                               ctypes.byref(n_pairs), ctypes.byref(n_hits)))
    n = n_pairs.value
    return oq[:n].copy(), orr[:n].copy(), os_[:n].copy(), n_hits.value


def same_hits(a, b):
    assert len(a[2]) == len(b[2])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))


def check_all_queries(orc, sq, flat, q, r, metric, Ks, ks, radii):
    """every query kind on the SQfp16 index of r against the oracle on dec(r) and the Flat index of dec(r)"""
    rd = dec(r)
    for K in Ks:
        got, ref = sq.global_topk(q, K), flat.global_topk(q, K)
        oi, oj, os_, info = orc.global_threshold_search(q, rd, K, metric, return_info=True)
        same_hits(got, (oi, oj, os_))
        same_hits(got, ref)
        assert np.float32(got[3]) == np.float32(info["radius"]) == np.float32(ref[3])
    for radius in radii:
        lims, D, I = sq.range_search(q, radius)
        ol, oD, oI = orc.range_search(q, rd, radius, metric)
        fl, fD, fI = flat.range_search(q, radius)
        assert len(D) > 0
        assert np.array_equal(lims, ol) and np.array_equal(I, oI) and np.array_equal(bits(D), bits(oD))
        assert np.array_equal(lims, fl) and np.array_equal(I, fI) and np.array_equal(bits(D), bits(fD))
    for k in ks:
        D, I = sq.search(q, k)
        oD, oI = orc.knn(q, rd, k, metric)
        fD, fI = flat.search(q, k)
        assert np.array_equal(I, oI) and np.array_equal(bits(D), bits(oD))
        assert np.array_equal(I, fI) and np.array_equal(bits(D), bits(fD))


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_equals_flat_on_decoded_rows(gpu, orc, route):
    opts, d, kind, proof = ROUTES[route]
    q, r = route_rows(route)
    rd = dec(r)
    sq, flat = make(d, "SQfp16", opts), make(d, "Flat", opts)
    sq.add(r[:1000]); sq.add(r[1000:])
    flat.add(rd)
    s_all = orc.scores(q, rd)
    srt = np.sort(s_all.ravel())[::-1]
    # K cuts inside groups of equal scores (the set is built for that) and one that takes most of the matrix
    tied = np.flatnonzero(srt[:-1] == srt[1:]) + 1   # cuts K with srt[K - 1] == srt[K]
    assert len(tied) > 100, "the set holds no ties"
    Ks = [1, int(tied[np.searchsorted(tied, 300)]), int(tied[np.searchsorted(tied, 4000)]), 1200 * 12]
    assert srt[Ks[1] - 1] == srt[Ks[1]] and srt[Ks[2] - 1] == srt[Ks[2]] and Ks[2] < 40000
    check_all_queries(orc, sq, flat, q, r, IP, Ks, [1, 5, 20, 100], [float(srt[2000]), float(srt[20])])
    st = sq.profile_read(reset=True)
    if proof == "i8":
        assert st["i8_launches"] > 0 and sq.get_option("i8_fallbacks") == 0, st
        assert st["rescore_launches"] > 0
    elif proof == "f16":
        assert st["f16_launches"] > 0 and st["i8_launches"] == 0 and st["rescore_launches"] > 0, st
    elif proof == "sim":
        assert st["sim_launches"] > 0 and st["f16_launches"] == 0 and st["i8_launches"] == 0, st
    if kind == "excluded":
        assert sq.get_option("i8") == 2.0
    if kind == "centred":
        assert sq.get_option("i8_center_on") == 1.0
    # candidates: (query video, reference video) max aggregation of the top-K hits
    row2q = (np.arange(len(q)) // 7).astype(np.int32)
    row2r = (np.arange(len(r)) // 11).astype(np.int32)
    for K in (300, 4000):
        a, b = candidates(sq, q, K, row2q, row2r), candidates(flat, q, K, row2q, row2r)
        same_hits(a, b)
        assert a[3] == b[3]
        oi, oj, os_ = orc.global_threshold_search(q, rd, K, IP)
        pq, pr, ps, _ = orc.pair_max(oi, oj, os_, row2q, row2r)
        order_a, order_o = np.lexsort((a[1], a[0])), np.lexsort((pr, pq))
        same_hits((a[0][order_a], a[1][order_a], a[2][order_a]), (pq[order_o], pr[order_o], ps[order_o]))


@pytest.mark.parametrize("d", [16, 100])
def test_l2_equals_flat_on_decoded_rows(gpu, orc, d):
    q, r = cr.with_ties(41, 120, 900, d)
    sq, flat = make(d, "SQfp16", metric=L2, rows=r), make(d, "Flat", metric=L2, rows=dec(r))
    D1, _ = flat.search(q, 3)
    radii = [float(np.median(D1[:, 2])), float(D1[:, 0].max()) + 1e-3]
    check_all_queries(orc, sq, flat, q, r, L2, [1, 200, 3000], [1, 3, 20, 70], radii)
    # (an L2 index keeps no pre-filter images: at these dims the store, padded to 128 columns, is no smaller than the
    # packed fp32 rows, padded to 64)


def test_exact_kernels_over_several_decoded_ranges(gpu, orc):
    """More rows than one decoded range of the exact readers holds (65536): the pre-filter-off search and the exact k-NN
    run range by range, hits and lists carry the ranges' offsets; the best matches are planted in the LAST range."""
    d, nq, nr = 16, 150, 70001
    q, r = cr.rows(51, nq, d), cr.rows(52, nr, d)
    r[nr - nq:] = q[::-1] * np.float32(0.999)
    r[66000:66020] = q[:20]
    rd = dec(r)
    for opts in (dict(prefilter=0), dict(prefilter=2, i8=2)):
        sq, flat = make(d, "SQfp16", opts, rows=r), make(d, "Flat", opts, rows=rd)
        check_all_queries(orc, sq, flat, q, r, IP, [1, 170, 5000], [1, 5, 100], [0.97])
        D, I = sq.search(q, 1)
        assert (I[:, 0] >= 65536).mean() > 0.8   # (the rest: rows that hold the large planted values of codec_rows)


def test_int8_upkeep_over_several_decoded_ranges(gpu, orc):
    """The int8 image's upkeep (per-coordinate min / max, centre, quantisation) reads an SQfp16 store in decoded ranges
    of 65536 rows and a Flat index in one piece: 65536 + 640 rows, one coordinate constant (excluded), centring forced,
    added in two calls that split at row 65000.  The upkeep is lazy -- the first search catches up on every row added
    so far -- so with both adds first it walks [0, 66176) as the ranges [0, 65536) and [65536, 66176); with a search
    between the adds (second leg) the catch-up of the second add starts at row 65000, not at a range boundary.
    Both walks must leave the same excluded set, centre and int8 image: the searches are bit-identical AND the global
    top-K and the k-NN hand the same number of candidates to the exact stage.  (A range search does not write the
    candidate counter; there the results and the int8 launches are compared.  No option reports the excluded set
    itself: a coordinate kept in one index's image and left out of the other's would show in the candidate counts.)"""
    d, nq, nr = 32, 256, 65536 + 640
    q, r = cr.rows(71, nq, d), cr.rows(72, nr, d)
    r[:, 5] = np.float32(0.7001)   # (not a half: the agreement must hold on the DECODED values)
    q[::4] = r[65300:65300 + nq // 4] * np.float32(0.999)   # best matches on both sides of the range boundary
    q[1::8] = r[65600:65600 + nq // 8]
    rd = dec(r)
    opts = dict(prefilter=2, i8=2, i8_center=2)
    sq, flat = make(d, "SQfp16", opts), make(d, "Flat", opts)
    sq.add(r[:65000]); sq.add(r[65000:])
    flat.add(rd[:65000]); flat.add(rd[65000:])
    srt = np.sort(orc.scores(q, rd).ravel())[::-1]

    def same_work(what, sq=sq, flat=flat, counts_candidates=True):
        a, b = sq.profile_read(reset=True), flat.profile_read(reset=True)
        print(f"\n{what}: candidates SQfp16 {a['candidates']}, Flat {b['candidates']}; int8 launches {a['i8_launches']} / {b['i8_launches']}")
        if counts_candidates:
            assert a["candidates"] == b["candidates"] and a["candidates"] > 0, (what, a["candidates"], b["candidates"])
        assert a["i8_launches"] > 0 and b["i8_launches"] > 0 and a["i8_launches"] == b["i8_launches"], (what, a, b)
        assert sq.get_option("i8_fallbacks") == 0 and flat.get_option("i8_fallbacks") == 0

    K = 3000
    got, ref = sq.global_topk(q, K), flat.global_topk(q, K)
    oi, oj, os_, info = orc.global_threshold_search(q, rd, K, IP, return_info=True)
    same_hits(got, (oi, oj, os_))
    same_hits(got, ref)
    assert np.float32(got[3]) == np.float32(info["radius"]) == np.float32(ref[3])
    same_work("global top-K")
    assert sq.get_option("i8_center_on") == 1.0 and flat.get_option("i8_center_on") == 1.0

    radius = float(srt[2000])
    lims, D, I = sq.range_search(q, radius)
    ol, oD, oI = orc.range_search(q, rd, radius, IP)
    fl, fD, fI = flat.range_search(q, radius)
    assert len(D) > 0 and (I >= 65536).any() and (I < 65536).any()
    assert np.array_equal(lims, ol) and np.array_equal(I, oI) and np.array_equal(bits(D), bits(oD))
    assert np.array_equal(lims, fl) and np.array_equal(I, fI) and np.array_equal(bits(D), bits(fD))
    same_work("range search", counts_candidates=False)

    for k in (1, 5):
        D, I = sq.search(q, k)
        oD, oI = orc.knn(q, rd, k, IP)
        fD, fI = flat.search(q, k)
        assert np.array_equal(I, oI) and np.array_equal(bits(D), bits(oD))
        assert np.array_equal(I, fI) and np.array_equal(bits(D), bits(fD))
        same_work(f"k-NN k = {k}")

    # second leg: a search between the two adds, so that the second add's catch-up starts at row 65000
    sq2, flat2 = make(d, "SQfp16", opts, rows=r[:65000]), make(d, "Flat", opts, rows=rd[:65000])
    D, I = sq2.search(q, 1)
    oD, oI = orc.knn(q, rd[:65000], 1, IP)
    fD, fI = flat2.search(q, 1)
    assert np.array_equal(I, oI) and np.array_equal(bits(D), bits(oD))
    assert np.array_equal(I, fI) and np.array_equal(bits(D), bits(fD))
    same_work("k-NN k = 1 on the first add", sq2, flat2)
    sq2.add(r[65000:]); flat2.add(rd[65000:])
    got, ref = sq2.global_topk(q, K), flat2.global_topk(q, K)
    same_hits(got, (oi, oj, os_))
    same_hits(got, ref)
    same_work("global top-K after the second add", sq2, flat2)


# ------------------------------------------------------------------------------------------------ 3. not an alias
@pytest.mark.parametrize("d", [256, 512])
def test_codec_rounds_and_halves_the_memory(gpu, d):
    """On rows that are not fp16-exact the codec's results differ from the Flat index of the same rows (it is not an
    alias of it), and it keeps less than half the bytes: 1556 against 3604 per 512-d row with both pre-filter images
    (0.43; the slack covers capacity rounding).  At small dims the ratio is larger, because the fp16 and int8 images
    pad their rows to 128 / 256 columns while the packed fp32 rows pad to 64."""
    rng = np.random.default_rng(8)
    q, x = cr.unit(rng, 200, d), cr.unit(rng, 6000, d)
    sq, flat = make(d, "SQfp16", rows=x), make(d, "Flat", rows=x)
    a, b = sq.global_topk(q, 3000), flat.global_topk(q, 3000)
    assert not np.array_equal(bits(a[2]), bits(b[2]))
    Da, _ = sq.search(q, 5)
    Db, _ = flat.search(q, 5)
    assert not np.array_equal(bits(Da), bits(Db))
    sb, fb = sq.get_option("ref_bytes"), flat.get_option("ref_bytes")
    assert sb > 0 and sb <= 0.5 * fb, (sb, fb, sb / fb)
    assert abs(sb / fb - 0.43) < 0.03, (sb, fb)


# ------------------------------------------------------------------------------------------------ 4. lossless on fp16 data
def _videos(x, lens, prefix, cls, dtype=np.float32):
    cuts = np.r_[0, np.cumsum(lens)]
    return [cls(video_id=f"{prefix}{k:05d}", timestamps=np.arange(lens[k], dtype=np.float32), feature=x[cuts[k]:cuts[k + 1]].astype(dtype))
            for k in range(len(lens))]


def test_fp16_exact_descriptors_lose_nothing(gpu, orc):
    import torch
    from helpers import flatten_pairmatches
    from vsc2022_amd import synth
    from vsc2022_amd.engine import DeviceMatcher, DeviceScoreNormalizer
    from vsc2022_amd.vsc.candidates import CandidateGeneration, MaxScoreAggregation
    from vsc2022_amd.vsc.index import VideoFeature, VideoIndex

    qv, rv, _ = synth.make_dataset(seed=23, n_query=30, n_ref=70, dim=256, q_frames=(8, 30), r_frames=(8, 40), planted_frac=0.4,
                                   static_frac=0.1)
    qv, rv = synth.to_video_features(qv, VideoFeature), synth.to_video_features(rv, VideoFeature)
    for v in qv + rv:
        v.feature = dec(v.feature)   # what a descriptor file written with --store_fp16 holds
    q16 = [VideoFeature(video_id=v.video_id, timestamps=v.timestamps, feature=v.feature.astype(np.float16)) for v in qv]
    r16 = [VideoFeature(video_id=v.video_id, timestamps=v.timestamps, feature=v.feature.astype(np.float16)) for v in rv]
    res = {}
    for codec, refs in (("Flat", rv), ("SQfp16", rv), ("SQfp16-half", r16), ("Flat-half", r16)):
        vi = VideoIndex(256, codec.split("-")[0])
        vi.add(refs[:30]); vi.add(refs[30:])
        cg = CandidateGeneration(refs[:1], MaxScoreAggregation())
        cg.index = vi
        out = []
        for K in (50, 1200 * 30):
            out.append([np.asarray(a).tolist() for a in flatten_pairmatches(vi.search(q16 if "half" in codec else qv, K))])
            out.append([(c.query_id, c.ref_id, np.float32(c.score).view(np.uint32)) for c in cg.query(qv, K)])
        out.append([np.asarray(a).tolist() for a in flatten_pairmatches(vi.search(qv, -3))])
        res[codec] = out
    for codec in ("SQfp16", "SQfp16-half", "Flat-half"):
        assert res[codec] == res["Flat"], codec

    qf, rf = np.concatenate([v.feature for v in qv]), np.concatenate([v.feature for v in rv])
    qoff = np.r_[0, np.cumsum([len(v.feature) for v in qv])].astype(np.int64)
    roff = np.r_[0, np.cumsum([len(v.feature) for v in rv])].astype(np.int64)

    def match(codec, qx, rx, bias=0.0):
        m = DeviceMatcher(rx, roff, 0, codec=codec)
        assert m.index.codec == codec
        m.set_queries(qx, qoff)
        r = m.match(bias=bias)
        return [t.cpu().numpy().copy() for t in (r.cand_q, r.cand_r, r.cand_score, r.nbox, r.boxes, r.box_score)] + [r.n_hits, r.radius]

    def same(a, b):
        for x, y in zip(a, b):
            if isinstance(x, np.ndarray) and x.dtype == np.float32:
                assert np.array_equal(bits(x), bits(y))
            else:
                assert np.array_equal(x, y)

    same(match("SQfp16", qf, rf), match("Flat", qf, rf))
    # score normalisation re-normalises the rows: its outputs are not fp16-exact.  The normalised references go
    # through dec before both matchers are built
    noise = dec(np.concatenate([np.asarray(v.feature, dtype=np.float32)
                                for v in synth.make_videos(np.random.default_rng(5), 20, 256, (20, 20), "N")]))
    tn = torch.from_numpy(noise).cuda()
    norm = DeviceScoreNormalizer(tn)
    qn = norm.queries(torch.from_numpy(qf).cuda()).cpu().numpy()
    rn = dec(norm.refs(torch.from_numpy(rf).cuda()).cpu().numpy())
    same(match("SQfp16", qn, rn, bias=0.5), match("Flat", qn, rn, bias=0.5))
    # the noise index: fp16-exact noise rows, no re-normalisation -> the same bias column
    a = DeviceScoreNormalizer(tn, l2_normalize=False, codec="SQfp16")
    b = DeviceScoreNormalizer(tn, l2_normalize=False, codec="Flat")
    assert a.noise_index.codec == "SQfp16" and a.noise_index.get_option("ref_bytes") < b.noise_index.get_option("ref_bytes")
    qa, qb = a.queries(torch.from_numpy(qf).cuda()), b.queries(torch.from_numpy(qf).cuda())
    assert torch.equal(qa.view(torch.int32), qb.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 5. incremental use
def test_adds_interleaved_with_searches(gpu, orc):
    """The int8 image follows the DECODED rows as they arrive: the excluded set shrinks with a later add, and the centre
    is decided when the index crosses 1024 rows (tests/test_gpu_i8.py shows the Flat form of both)."""
    d = 96
    q, r = cr.rows(61, 400, d), cr.rows(62, 2600, d)
    const = {3: 0.7001, 10: -1.5, 11: 2.0, 20: 0.2503, 40: 30.0}
    for c, v in const.items():
        r[:, c] = np.float32(v)
    r[1800:, 10] = 0.3
    r[1800:, 40] = -2.0
    q[:, 40] *= 0.05
    for opts in (dict(prefilter=2, i8=2), dict(prefilter=2, i8=2, i8_center=1), {}):
        idx = make(d, "SQfp16", opts)
        for lo, hi, K in ((0, 500, 400), (500, 900, 700), (900, 1800, 1500), (1800, 2600, 2500)):
            idx.add(r[lo:hi])
            rd = dec(r[:hi])
            same_hits(idx.global_topk(q, K), orc.global_threshold_search(q, rd, K))
            D, I = idx.search(q, 3)
            oD, oI = orc.knn(q, rd, 3)
            assert np.array_equal(I, oI) and np.array_equal(bits(D), bits(oD))
            assert np.array_equal(bits(idx.reconstruct_n(lo, hi - lo)), bits(rd[lo:hi]))
        lims, Dr, Ir = idx.range_search(q, 0.5)
        ol, oD, oI = orc.range_search(q, dec(r), 0.5)
        assert np.array_equal(lims, ol) and np.array_equal(Ir, oI) and np.array_equal(bits(Dr), bits(oD))
        if opts:
            assert idx.profile_read()["i8_launches"] > 0
    # rows with a common direction: the centre switches on at the add that crosses 1024 rows
    qs, rs = shifted_rows(63, 300, 128), shifted_rows(64, 2000, 128)
    idx = make(128, "SQfp16", dict(prefilter=2, i8=2, i8_center=1))
    for lo, hi in ((0, 700), (700, 1500), (1500, 2000)):
        idx.add(rs[lo:hi])
        same_hits(idx.global_topk(qs, 900), orc.global_threshold_search(qs, dec(rs[:hi]), 900))
        assert idx.get_option("i8_center_on") == (1.0 if hi >= 1024 else 0.0)


# ------------------------------------------------------------------------------------------------ 6. full size
@pytest.fixture(scope="module")
def fullsize(gpu):
    import torch
    from bench import plant_copies, synth_on_device

    dev = torch.device("cuda", 0)
    n_qv, qf, n_rv, rf, dim = 8000, 25, 40000, 50, 512
    refs = synth_on_device(torch, dev, 1, n_rv, rf, dim)
    queries = synth_on_device(torch, dev, 1001, n_qv, qf, dim)
    plant_copies(torch, dev, 2001, queries, n_qv, qf, refs, n_rv, rf)
    return queries, refs, 1200 * n_qv


def test_fullsize_equals_flat_on_decoded_rows(fullsize):
    """200 k query x 2 M reference rows, 512-d, K = 9.6 M, default routing: the whole hit table and the 1-NN column."""
    import torch

    queries, refs, K = fullsize
    out = {}
    for codec in ("SQfp16", "Flat"):
        idx = make(512, codec)
        idx.use_torch_stream()
        idx.add(refs if codec == "SQfp16" else refs.to(torch.float16).to(torch.float32))
        i, j, s, radius = idx.global_topk(queries, K, device_out=True)
        D, I = idx.search(queries, 1, device_out=True)
        out[codec] = (i.clone(), j.clone(), s.clone(), radius, D.clone(), I.clone(), idx.get_option("ref_bytes"), idx.profile_read())
        del idx
        torch.cuda.empty_cache()
    a, b = out["SQfp16"], out["Flat"]
    assert a[2].numel() == K and a[3] == b[3]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    assert torch.equal(a[5], b[5]) and torch.equal(a[4].view(torch.int32), b[4].view(torch.int32))
    assert a[6] <= 0.5 * b[6], (a[6], b[6])
    assert a[7]["i8_launches"] > 0 and a[7]["rescore_launches"] > 0
    print(f"\nref_bytes SQfp16 {a[6] / 2**30:.2f} GiB, Flat {b[6] / 2**30:.2f} GiB; exact stage {a[7]['rescore_ms']:.1f} / {b[7]['rescore_ms']:.1f} ms")


@pytest.mark.parametrize("kind,opts", [("i8", dict(prefilter=2, i8=2)), ("f16", dict(prefilter=2, i8=0))])
def test_planted_bound_rows_through_the_codec(gpu, orc, kind, opts):
    """tests/prefilter_bounds.py's planted rows (512-d), passed through dec: results equal the oracle on the decoded rows.
    The share of the pre-filter's bound that the planted pairs still reach after rounding is PRINTED, not asserted:
    rounding the references to 11 bits necessarily blunts the int8 construction (its residuals of 63/128 of a step no
    longer line up); it tells a reader how hard this leg pushes."""
    c = pb.topk_case(kind, 512)
    rows, refs = c.planted()
    cd = pb.Case(c.q, dec(c.r), c.partner, c.kind, c.d, c.exclude, c.mu)
    before, after = pb.PairBound(c, rows, refs).reach()[0], pb.PairBound(cd, rows, refs).reach()[0]
    print(f"\n{kind}: planted pairs reach {np.abs(before).min():.3f}..{np.abs(before).max():.3f} of the bound as built, "
          f"{np.abs(after).min():.3f}..{np.abs(after).max():.3f} after the references went through dec")
    sq, flat = make(512, "SQfp16", opts, rows=c.r), make(512, "Flat", opts, rows=cd.r)
    s = orc.scores(c.q[rows[:1]], cd.r[refs[:1]])[0, 0]
    check_all_queries(orc, sq, flat, c.q, c.r, IP, [c.K, 4 * c.K], [1, 5], [float(np.nextafter(s, np.float32(-np.inf)))])
    st = sq.profile_read()
    assert st["i8_launches" if kind == "i8" else "f16_launches"] > 0
