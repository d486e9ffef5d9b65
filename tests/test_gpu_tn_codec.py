"""The SQfp16 reference codec of the Temporal-Network context on the GPU: a context whose references are the rows X,
kept as half floats, behaves bit for bit as the Flat context on dec(X) = X.astype(float16).astype(float32) -- boxes,
box counts, MaxSim score bits and similarity-matrix bits -- whatever form the rows are handed over in.  Every equality
is exact.
"""
import ctypes
import functools

import numpy as np
import pytest

import codec_rows as cr
from codec_rows import dec
from helpers import bits

pytestmark = pytest.mark.gpu

FLAT, SQ = "Flat", "SQfp16"
# the reference's two parameter sets: VCSL's defaults, and what sscd_baseline.py passes
PARAM_SETS = ((0.0, {}), (0.5, dict(tn_max_step=5, min_length=4)))
# video lengths around the 32-row MFMA block and the 64-column two-block pass; a zero-length video on both sides; the
# LAST reference video ends in a single block after a two-block pass (its rows are the last of the store)
Q_LENS = (5, 0, 33, 64, 1, 97, 31, 65, 32, 63, 5, 33)
R_LENS = (32, 65, 0, 1, 97, 63, 5, 64, 31, 33, 97, 65)
DIMS = (16, 100, 512, 513, 768)


def offsets(lens):
    return np.ascontiguousarray(np.r_[0, np.cumsum(lens)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def video_set(d, q_lens=Q_LENS, r_lens=R_LENS):
    """(q rows, q offsets, r rows, r offsets): codec_rows rows (unit-norm Gaussian + the values a wrong rounding misses)
    with noisy copies of reference segments planted into the queries, so that both parameter sets find boxes."""
    q_off, r_off = offsets(q_lens), offsets(r_lens)
    q, r = cr.rows(1000 + d, int(q_off[-1]), d), cr.rows(2000 + d, int(r_off[-1]), d)
    assert not np.array_equal(dec(r), r)  # the rounding changes the rows: equality with Flat on X would not hold
    rng = np.random.default_rng(d)
    for qv, rv in ((2, 0), (3, 1), (5, 4), (7, 11), (9, 7), (11, 11), (6, 8)):
        if qv >= len(q_lens):
            continue
        n = min(q_lens[qv], r_lens[rv]) - 2
        seg = r[r_off[rv] + 1:r_off[rv] + 1 + n] + (0.3 / np.sqrt(d)) * rng.standard_normal((n, d)).astype(np.float32)
        q[q_off[qv] + 2:q_off[qv] + 2 + n] = seg / np.linalg.norm(seg, axis=1, keepdims=True)
    q.setflags(write=False), r.setflags(write=False)
    return q, q_off, r, r_off


class Ctx:
    """A libvscmi TN context over numpy / torch rows (fp32 queries; fp32 or fp16 references, host or HBM)."""

    def __init__(self, q, q_off, r, r_off, codec, dim):
        from vsc2022_amd import _lib

        self.L, self._lib = _lib.lib(), _lib
        self.q_off, self.r_off = q_off, r_off
        self.h = ctypes.c_void_p()
        self._keep = (q, r)
        qp, q_mem = _lib.ptr(q)
        rp, r_mem = _lib.ptr(r)
        r_f16 = "float16" in str(r.dtype)
        _lib.check(self.L.vsc_tn_create_codec(qp if len(q) else None, q_off.ctypes.data, len(q_off) - 1,
                                              rp if len(r) else None, int(r_f16), r_off.ctypes.data, len(r_off) - 1,
                                              dim, q_mem, r_mem, _lib.CODECS[codec], 0, ctypes.byref(self.h)))
        assert self.h.value

    def set_queries(self, q, q_off):
        self.q_off, self._keep = q_off, (q, self._keep[1])
        qp, q_mem = self._lib.ptr(q)
        self._lib.check(self.L.vsc_tn_set_queries(self.h, qp, q_off.ctypes.data, len(q_off) - 1, q_mem))

    def ref_bytes(self):
        return int(self.L.vsc_tn_ref_bytes(self.h))

    def localize(self, bias=0.0, pairs=None, **kw):
        """All pairs (or `pairs`) -> (n_boxes, the valid boxes of every pair in one array, the bits of their scores)."""
        from vsc2022_amd.vcsl.vta import tn_params

        nq, nr = len(self.q_off) - 1, len(self.r_off) - 1
        if pairs is None:
            pairs = [(a, b) for a in range(nq) for b in range(nr)]
        pq = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int32)
        pr = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int32)
        n = len(pairs)
        nb = np.zeros(n, np.int32)
        boxes = np.zeros((n, self._lib.TN_MAX_BOXES, 4), np.int32)
        bmax = np.zeros((n, self._lib.TN_MAX_BOXES), np.float32)
        prm = tn_params(**kw)
        self._lib.check(self.L.vsc_tn_localize(self.h, pq.ctypes.data, pr.ctypes.data, n, self._lib.MEM_HOST, ctypes.byref(prm),
                                               float(bias), nb.ctypes.data, boxes.ctypes.data, bmax.ctypes.data,
                                               self._lib.MEM_HOST))
        valid = np.arange(self._lib.TN_MAX_BOXES)[None, :] < nb[:, None]
        return nb, boxes[valid], bits(bmax[valid])

    def similarity(self, qv, rv, bias=0.0):
        lq, lr = int(self.q_off[qv + 1] - self.q_off[qv]), int(self.r_off[rv + 1] - self.r_off[rv])
        out = np.zeros((lq, lr), np.float32)
        a, b = ctypes.c_int32(0), ctypes.c_int32(0)
        self._lib.check(self.L.vsc_tn_similarity(self.h, qv, rv, float(bias), out.ctypes.data, out.size, ctypes.byref(a),
                                                 ctypes.byref(b)))
        assert (a.value, b.value) == (lq, lr)
        return out

    def close(self):
        if self.h.value:
            self.L.vsc_tn_destroy(self.h)
            self.h = ctypes.c_void_p()

    __del__ = close


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def flat_results(d):
    """The Flat context on dec(X): its results under both parameter sets (computed once per dim)."""
    q, q_off, r, r_off = video_set(d)
    ctx = Ctx(q, q_off, dec(r), r_off, FLAT, d)
    out = tuple(ctx.localize(bias, **kw) for bias, kw in PARAM_SETS)
    ctx.close()
    return out


SIM_PAIRS = ((0, 0), (5, 4), (len(Q_LENS) - 1, len(R_LENS) - 1))


# ----------------------------------------------------------------------------------- 1. equality with Flat on dec(X)
@pytest.mark.parametrize("d", DIMS)
def test_sqfp16_context_equals_flat_on_decoded_rows(gpu, d):
    import torch

    q, q_off, r, r_off = video_set(d)
    want = flat_results(d)
    assert sum(int(w[0].sum()) for w in want) >= 8, "too few boxes for the comparison to mean anything"
    assert want[0][0][1 * len(R_LENS) + 3] == 0 and want[0][0][3 * len(R_LENS) + 2] == 0  # (zero-length videos)
    assert max(int(w[0][-1]) for w in want) >= 1, "the pair of the LAST reference video has no box"
    flat_dec = Ctx(q, q_off, dec(r), r_off, FLAT, d)
    flat_raw = Ctx(q, q_off, r, r_off, FLAT, d)
    half = r.astype(np.float16)
    sources = (r, torch.from_numpy(np.array(r)).cuda(), half, torch.from_numpy(half).cuda())
    differs = False
    for src in sources:
        ctx = Ctx(q, q_off, src, r_off, SQ, d)
        for (bias, kw), w in zip(PARAM_SETS, want):
            assert same(ctx.localize(bias, **kw), w), (d, type(src), str(src.dtype), kw)
        for qv, rv in SIM_PAIRS:
            got = bits(ctx.similarity(qv, rv, 0.5))
            assert np.array_equal(got, bits(flat_dec.similarity(qv, rv, 0.5))), (d, qv, rv)
            differs |= not np.array_equal(got, bits(flat_raw.similarity(qv, rv, 0.5)))
        ctx.close()
    assert differs, "the SQfp16 context scores like the Flat context on the UNDECODED rows: nothing was rounded"
    # a Flat context takes half rows too: the context of the upcast array
    for src in (half, torch.from_numpy(half).cuda()):
        ctx = Ctx(q, q_off, src, r_off, FLAT, d)
        assert same(ctx.localize(*PARAM_SETS[1][:1], **PARAM_SETS[1][1]), want[1])
        ctx.close()
    flat_dec.close(), flat_raw.close()


# ------------------------------------------------------------------------------------------ 2. CPU oracle on dec(X)
def test_sqfp16_context_equals_the_cpu_oracle_on_decoded_rows(gpu, orc):
    d = 512
    q, q_off, r, r_off = video_set(d)
    rd = dec(r)
    ctx = Ctx(q, q_off, r.astype(np.float16), r_off, SQ, d)
    n_boxes = 0
    for bias, kw in PARAM_SETS:
        nb, boxes, sbits = ctx.localize(bias, **kw)
        exp_nb, exp_boxes, exp_bits = [], [], []
        for a in range(len(Q_LENS)):
            for b in range(len(R_LENS)):
                qa, rb = q[q_off[a]:q_off[a + 1]], rd[r_off[b]:r_off[b + 1]]
                found = []
                if len(qa) and len(rb):
                    sims = orc.pair_sims(qa, rb, bias)
                    if (a, b) in SIM_PAIRS:
                        assert np.array_equal(bits(ctx.similarity(a, b, bias)), bits(sims))
                    found = orc.tn(sims, **kw)
                    exp_bits += [np.float32(sims[x1:x2, y1:y2].max() - np.float32(bias)) for (x1, y1, x2, y2) in found]
                exp_nb.append(len(found))
                exp_boxes += [list(f) for f in found]
        assert np.array_equal(nb, np.array(exp_nb, np.int32))
        assert np.array_equal(boxes, np.array(exp_boxes, np.int32).reshape(-1, 4))
        assert np.array_equal(sbits, bits(np.array(exp_bits, np.float32)))
        n_boxes += len(exp_boxes)
    assert n_boxes >= 8
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. HBM-state route
def test_sqfp16_over_long_video_runs_from_hbm_state(gpu):
    """A 1400-frame query video: its working state does not fit the LDS (tn_pair_kernel<int, true>: state and
    similarity slab in HBM), next to ordinary pairs in the same call."""
    d = 64
    q_lens, r_lens = (1400, 30), (900, 40)
    q_off, r_off = offsets(q_lens), offsets(r_lens)
    q, r = cr.rows(31, int(q_off[-1]), d), cr.rows(32, int(r_off[-1]), d)
    assert not np.array_equal(dec(r), r)
    rng = np.random.default_rng(8)
    seg = r[100:500] + 0.05 * rng.standard_normal((400, d)).astype(np.float32)
    q[700:1100] = seg / np.linalg.norm(seg, axis=1, keepdims=True)
    flat, sq = Ctx(q, q_off, dec(r), r_off, FLAT, d), Ctx(q, q_off, r, r_off, SQ, d)
    for bias, kw in PARAM_SETS:
        want = flat.localize(bias, **kw)
        assert want[0][0] >= 1
        assert same(sq.localize(bias, **kw), want)
    assert np.array_equal(bits(sq.similarity(0, 0, 0.5)), bits(flat.similarity(0, 0, 0.5)))
    flat.close(), sq.close()


# ------------------------------------------------------------------------------- 4. new queries, resident references
def test_set_queries_on_an_sqfp16_context(gpu):
    d = 100
    q, q_off, r, r_off = video_set(d)
    longer = video_set(d, Q_LENS + (97, 64, 33), R_LENS)[:2]
    shorter = video_set(d, Q_LENS[:5], R_LENS)[:2]
    ctx = Ctx(q, q_off, r, r_off, SQ, d)
    bias, kw = PARAM_SETS[1]
    assert same(ctx.localize(bias, **kw), flat_results(d)[1])
    for nq, nq_off in (longer, shorter, (q, q_off)):
        ctx.set_queries(nq, nq_off)
        fresh = Ctx(nq, nq_off, r, r_off, SQ, d)
        want = fresh.localize(bias, **kw)
        assert int(want[0].sum()) >= 2
        assert same(ctx.localize(bias, **kw), want)
        assert np.array_equal(bits(ctx.similarity(2, 0)), bits(fresh.similarity(2, 0)))
        fresh.close()
    assert same(ctx.localize(bias, **kw), flat_results(d)[1])
    ctx.close()


# ------------------------------------------------------------------------------------------ 5. rows fp16 cannot hold
@pytest.mark.parametrize("bad", [1e5, -7e4, np.nan, np.inf])
def test_rows_fp16_cannot_hold_fail_the_create(gpu, bad):
    import torch

    d = 100
    q, q_off, r, r_off = video_set(d)
    y = np.array(r)
    y[len(y) - 3, d - 1] = bad
    sources = [y, torch.from_numpy(y).cuda()]
    if not np.isfinite(bad):
        sources += [y.astype(np.float16), torch.from_numpy(y.astype(np.float16)).cuda()]
    for src in sources:
        with pytest.raises(ValueError):
            Ctx(q, q_off, src, r_off, SQ, d)
    ctx = Ctx(q, q_off, r, r_off, SQ, d)
    for (bias, kw), w in zip(PARAM_SETS, flat_results(d)):
        assert same(ctx.localize(bias, **kw), w)
    ctx.close()


# --------------------------------------------------------------------------------------------------------- 6. bytes
@pytest.mark.parametrize("d", [100, 513])
def test_reference_bytes_halve(gpu, d):
    q, q_off, r, r_off = video_set(d)
    flat, sq = Ctx(q, q_off, r, r_off, FLAT, d), Ctx(q, q_off, r, r_off, SQ, d)
    r_rows = (int(r_off[-1]) + 32 + 127) // 128 * 128   # + the slack of the last video's blocks, rounded to 128 rows
    dpad = (d + 63) // 64 * 64
    assert flat.ref_bytes() == r_rows * dpad * 4
    assert sq.ref_bytes() * 2 == flat.ref_bytes()
    flat.close(), sq.close()


# ------------------------------------------------------------------------------------------------ 7. Python surface
def _videos(rows, off, prefix, conv=lambda x: x):
    from vsc2022_amd.vsc.index import VideoFeature

    out = []
    for v in range(len(off) - 1):
        n = int(off[v + 1] - off[v])
        ts = np.stack([np.arange(n, dtype=np.float32), np.arange(1, n + 1, dtype=np.float32)], axis=1)
        out.append(VideoFeature(video_id=f"{prefix}{v:06d}", timestamps=ts, feature=conv(np.array(rows[off[v]:off[v + 1]]))))
    return out


def _fields(matches):
    return [(m.query_id, m.ref_id, m.query_start, m.query_end, m.ref_start, m.ref_end, int(np.float32(m.score).view(np.uint32)))
            for m in matches]


def test_localization_classes_take_ref_codec(gpu):
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim
    from vsc2022_amd.vsc.metrics import CandidatePair

    d = 100
    q, q_off, r, r_off = video_set(d)
    qv = _videos(q, q_off, "Q")
    pairs = [CandidatePair(f"Q{a:06d}", f"R{b:06d}", 1.0) for a in range(len(Q_LENS)) for b in range(len(R_LENS))]
    kw = dict(similarity_bias=0.5, tn_max_step=5, min_length=4)

    class Hooked(VCSLLocalizationMaxSim):   # a score() the fused kernel cannot know: matrices on the host, box by box
        def score(self, candidate, match, box, similarity):
            x1, y1, x2, y2 = box
            return similarity[x1:x2, y1:y2].max() - self.similarity_bias

    for cls in (VCSLLocalizationMaxSim, Hooked):
        want_loc = cls(qv, _videos(r, r_off, "R", dec), "TN", **kw)
        want = _fields(want_loc.localize_all(pairs))
        assert len(want) >= 4
        for conv in (lambda x: x, lambda x: x.astype(np.float16)):   # fp32 features, and features that are half rows
            loc = cls(qv, _videos(r, r_off, "R", conv), "TN", ref_codec=SQ, **kw)
            assert loc.ref_codec == SQ and loc.ref_bytes * 2 == want_loc.ref_bytes
            assert _fields(loc.localize_all(pairs)) == want
        raw = _fields(cls(qv, _videos(r, r_off, "R"), "TN", **kw).localize_all(pairs))
        assert raw != want   # (the default still localises on the rows as they are)


def test_device_matcher_tn_codec(gpu):
    import torch

    from vsc2022_amd.engine import DeviceMatcher

    d = 100
    lens_q = tuple(Q_LENS[k % len(Q_LENS)] for k in range(30))
    lens_r = tuple(R_LENS[k % len(R_LENS)] for k in range(30))
    q, q_off, r, r_off = video_set(d, lens_q, lens_r)
    pq, pr = (t.reshape(-1).contiguous() for t in torch.meshgrid(torch.arange(30, dtype=torch.int32, device="cuda"),
                                                                 torch.arange(30, dtype=torch.int32, device="cuda"),
                                                                 indexing="ij"))

    def run(refs, **kw):
        m = DeviceMatcher(refs, r_off, **kw)
        m.set_queries(np.array(q), q_off)
        nb, boxes, bmax = (t.cpu().numpy() for t in m.localize(pq, pr, bias=0.5))
        valid = np.arange(boxes.shape[1])[None, :] < nb[:, None]
        return nb, boxes[valid], bits(bmax[valid])

    on_dec, on_raw = run(dec(r)), run(np.array(r))
    assert int(on_dec[0].sum()) >= 8 and not same(on_dec, on_raw)
    assert same(run(np.array(r), tn_codec=SQ), on_dec)
    # `codec` keeps meaning the index only: the aligner still sees the rows as they are
    assert same(run(np.array(r), codec=SQ), on_raw)
