"""The half-float store of DnS's attention fine descriptors on the device (vsc_tn_set_fine_f16, fine_sim_kernel<true>)
against the fp32 store of the decoded values and the CPU restatement in tests/dns_fine_ref.py: BIT PATTERNS throughout.
dec(X) = X.astype(float16).astype(float32) (dns_fine_ref.half_rounded); a half converts to fp32 exactly and the chain is
the same, so there is no tolerance anywhere (include/vscmi.h).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dns_fine_ref as ref
import helpers
from test_gpu_fine_bits import BitsCtx, _bin_inputs, _coarse, _same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16 = np.float32, np.float16
CANARY = F32(-7.25)  # what Ctx.fine_similarity fills the output with


class HalfCtx(BitsCtx):
    def set_fine_f16(self, qf, rf, src_f16, check=True, device=False):
        """qf / rf: lists of [L, R, D] arrays (None: that side is left alone), sent as fp32 (src_f16 = 0) or as halves."""
        def rows(fine):
            if fine is None:
                return None
            return np.ascontiguousarray(np.concatenate(fine, axis=0), dtype=F16 if src_f16 else F32)

        some = next(f for f in (qf or rf) if f is not None)
        q, r = rows(qf), rows(rf)
        mem, keep = self._lib.MEM_HOST, []
        addr = [None if x is None else x.ctypes.data for x in (q, r)]
        if device:
            import torch

            keep = [None if x is None else torch.from_numpy(x).to("cuda:0") for x in (q, r)]
            assert all(t is None or t.dtype == (torch.float16 if src_f16 else torch.float32) for t in keep)
            torch.cuda.synchronize()
            addr, mem = [None if t is None else t.data_ptr() for t in keep], self._lib.MEM_DEVICE
        rc = self.L.vsc_tn_set_fine_f16(self.ctx, addr[0], addr[1], some.shape[1], some.shape[2], int(src_f16), mem)
        if check:
            self._lib.check(rc)
        return rc

    def stage1(self, pairs, symmetric, device_out=True):
        rc, mats, out = self.fine_similarity(pairs, symmetric, device_out=device_out)
        assert rc == 0, self.L.vsc_last_error()
        assert not (out[:sum(m.size for m in mats)] == CANARY).any()  # every cell was written
        return mats


def tile_lens(regions):
    """With F = 64 // R frames per tile side: tiles end before, on and after a video's last frame, and the longest video
    is last on each side, so that its last tile reads the slack rows."""
    f = 64 // regions
    return (1, f, f + 1, 2 * f + 3), (f + 1, 1, 3 * f)


def all_pairs(q_lens, r_lens):
    return [(q, r) for q in range(len(q_lens)) for r in range(len(r_lens))]


def _att_inputs(seed, lens, regions, dim):
    """Unit rows in fp32: not representable as halves."""
    rng = np.random.default_rng(seed)
    return [ref.unit_rows(rng, n * regions, dim).reshape(n, regions, dim) for n in lens]


def dec(fine):
    return [ref.half_rounded(x) for x in fine]


def _four_ways(c, qf, rf, pairs):
    """Stage 1 of `pairs`, both values of `symmetric`: the half store from fp32 X == the ATT store from dec(X) == the
    restatement on dec(X) == the half store from X.astype(float16) handed over as halves."""
    qd, rd = dec(qf), dec(rf)
    want = {s: [ref.fine_sim(qd[q], rd[r], "att", s) for q, r in pairs] for s in (False, True)}
    c.set_fine_f16(qf, rf, 0)
    from_fp32 = {s: c.stage1(pairs, s) for s in (False, True)}
    c.set_fine(qd, rd, "att")
    from_att = {s: c.stage1(pairs, s) for s in (False, True)}
    c.set_fine_f16([x.astype(F16) for x in qf], [x.astype(F16) for x in rf], 1)
    from_f16 = {s: c.stage1(pairs, s, device_out=False) for s in (False, True)}
    for s in (False, True):
        _same_bits(pairs, from_fp32[s], want[s], "half store from fp32 / restatement", s)
        _same_bits(pairs, from_att[s], want[s], "ATT store of dec(X) / restatement", s)
        _same_bits(pairs, from_fp32[s], from_att[s], "half store from fp32 / ATT store of dec(X)", s)
        _same_bits(pairs, from_f16[s], from_att[s], "half store from halves / ATT store of dec(X)", s)
    return want


# ---- 1. stage 1 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regions,dim", [(1, 1), (3, 7), (9, 72), (16, 200), (9, 512)])
def test_stage1_four_ways(gpu, orc, regions, dim):
    """D = 7, 72, 200: k padding; D = 1: the degenerate chain."""
    q_lens, r_lens = tile_lens(regions)
    pairs = all_pairs(q_lens, r_lens)
    assert len(pairs) == 12
    qc, rc = _coarse(11, q_lens, r_lens)
    qf, rf = _att_inputs(regions * 1000 + dim, q_lens, regions, dim), _att_inputs(regions * 1000 + dim + 1, r_lens, regions, dim)
    if dim > 1:  # (a unit row of one element is +-1: a half already)
        assert any((ref.half_rounded(x) != x).any() for x in qf)
    c = HalfCtx(qc, rc)
    try:
        _four_ways(c, qf, rf, pairs)
    finally:
        c.close()


# ---- 2. extremes ----------------------------------------------------------------------------------------------------

def _extreme_inputs(seed, lens, regions=3, dim=8):
    """Rows of the largest halves of both signs, a half subnormal (6e-8 -> 2^-24), a value that rounds to zero (1e-9),
    -0.0 and ordinary values.  8 * 65504^2 < 3.5e10: every sum stays finite."""
    rng = np.random.default_rng(seed)
    palette = np.array([65504.0, -65504.0, 6e-8, -6e-8, 1e-9, -0.0, 0.0, 0.3333, -1.7], dtype=F32)
    return [palette[rng.integers(0, len(palette), size=(n, regions, dim))] for n in lens]


def test_extremes(gpu, orc):
    regions, dim = 3, 8
    q_lens, r_lens = tile_lens(regions)
    pairs = all_pairs(q_lens, r_lens)
    qf, rf = _extreme_inputs(5, q_lens), _extreme_inputs(6, r_lens)
    d = ref.half_rounded(np.array([6e-8, 1e-9, 65504.0], dtype=F32))
    assert d[0] == F32(2.0 ** -24) and d[1] == 0.0 and d[2] == 65504.0
    qc, rc = _coarse(12, q_lens, r_lens)
    c = HalfCtx(qc, rc)
    try:
        want = _four_ways(c, qf, rf, pairs)
        assert all(np.isfinite(m).all() for s in want for m in want[s])
    finally:
        c.close()


# ---- 3. memory and state --------------------------------------------------------------------------------------------

def _round_up(x, m):
    return (x + m - 1) // m * m


def _side_bytes(frames, regions, dim, esz=2):
    """64 rows of slack after the side's last row; rows padded to a multiple of 128 and values to a multiple of 64 like
    every row store of the engine (include/vscmi.h)."""
    return _round_up(frames * regions + 64, 128) * _round_up(dim, 64) * esz


def _refuses(c, pairs, side):
    from vsc2022_amd import _lib

    rc = c.fine_similarity(pairs, True)[0]
    assert rc == _lib.VSC_ERR_INVALID and ("no %s fine descriptors" % side).encode() in c.L.vsc_last_error(), c.L.vsc_last_error()


def test_memory(gpu):
    regions, dim = 9, 72
    q_lens, r_lens = tile_lens(regions)
    qc, rc = _coarse(13, q_lens, r_lens)
    qf, rf = _att_inputs(30, q_lens, regions, dim), _att_inputs(31, r_lens, regions, dim)
    c = HalfCtx(qc, rc)
    try:
        c.set_fine(qf, rf, "att")
        as_fp32 = c.fine_bytes()
        assert as_fp32 == _side_bytes(sum(q_lens), regions, dim, 4) + _side_bytes(sum(r_lens), regions, dim, 4)
        c.set_fine_f16(qf, rf, 0)
        assert c.fine_bytes() == _side_bytes(sum(q_lens), regions, dim) + _side_bytes(sum(r_lens), regions, dim)
        assert c.fine_bytes() * 2 == as_fp32
        c.set_fine_f16(None, rf, 1)  # one side again: the counter is per side, not cumulative
        assert c.fine_bytes() * 2 == as_fp32
    finally:
        c.close()
    # where frames R + 64 is a multiple of 128 no row padding is added: (frames R + 64) * round_up(fdim, 64) * 2 per side
    regions, dim, q_lens, r_lens = 16, 200, (1, 3), (4,)
    qc, rc = _coarse(14, q_lens, r_lens)
    c = HalfCtx(qc, rc)
    try:
        c.set_fine_f16(_att_inputs(32, q_lens, regions, dim), _att_inputs(33, r_lens, regions, dim), 0)
        assert c.fine_bytes() == 2 * (4 * 16 + 64) * 256 * 2
    finally:
        c.close()


def test_state(gpu, orc):
    """A NULL side keeps that side; vsc_tn_set_queries drops the query side; ATT -> F16 -> BITS -> F16 drops both sides
    each time, and stage 1 refuses until both are set again."""
    regions, dim = 4, 33
    q_lens, r_lens = (7, 8, 20, 0, 33), (9, 31, 1, 16)
    pairs = [(0, 0), (1, 1), (2, 2), (4, 1), (3, 0), (2, 3), (4, 3), (0, 2)]
    qc, rc = _coarse(15, q_lens, r_lens)
    qa, ra = _att_inputs(40, q_lens, regions, dim), _att_inputs(41, r_lens, regions, dim)
    ra2 = _att_inputs(42, r_lens, regions, dim)
    qb, rb = _bin_inputs(43, q_lens, regions, dim), _bin_inputs(44, r_lens, regions, dim)
    c = HalfCtx(qc, rc)

    def run(qf, rf, kind="att"):
        if kind == "att":
            qf, rf = dec(qf), dec(rf)
        for symmetric in (True, False):
            _same_bits(pairs, c.stage1(pairs, symmetric), [ref.fine_sim(qf[q], rf[r], kind, symmetric) for q, r in pairs], symmetric)

    try:
        c.set_fine(dec(qa), dec(ra), "att")
        run(qa, ra)
        c.set_fine_f16(qa, None, 0)  # ATT -> F16: the reference side's fp32 rows are gone
        _refuses(c, pairs, "reference")
        assert c.fine_bytes() == _side_bytes(sum(q_lens), regions, dim)
        c.set_fine_f16(None, ra, 1)
        run(qa, ra)
        c.set_fine_f16(None, ra2, 0)  # a NULL side keeps what it had
        run(qa, ra2)
        c.set_fine_bits(qb, None, 1)  # F16 -> BITS
        _refuses(c, pairs, "reference")
        c.set_fine_bits(None, rb, 0)
        run(qb, rb, "bin")
        c.set_fine_f16(None, ra, 0)  # BITS -> F16
        _refuses(c, pairs, "query")
        c.set_fine_f16(qa, None, 1)
        run(qa, ra)
        c.set_fine(None, dec(ra), "att")  # F16 -> ATT
        _refuses(c, pairs, "query")
        c.set_fine_f16(qa, ra, 0)
        # a new query side drops the query descriptors
        q_lens2 = (12, 0, 8, 9, 30)
        qc2, _ = _coarse(16, q_lens2, r_lens)
        c.set_queries(qc2)
        _refuses(c, pairs, "query")
        assert c.fine_bytes() == _side_bytes(sum(r_lens), regions, dim)
        qa2 = _att_inputs(45, q_lens2, regions, dim)
        c.set_fine_f16(qa2, None, 0)
        pairs[:] = [(0, 0), (2, 1), (4, 3), (1, 2), (3, 3)]
        run(qa2, ra)
    finally:
        c.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------

def _refusal_sequence():
    """Argument checks on finite memory: a source element a half cannot hold is VSC_ERR_INVALID, the written side is gone
    (no descriptors, no bytes), the other side is still usable, and a following good call on the same handle returns the
    right bits."""
    import oracle as orc
    from vsc2022_amd import _lib

    orc.build()
    regions, dim = 3, 7
    q_lens, r_lens = tile_lens(regions)
    pairs = all_pairs(q_lens, r_lens)
    qc, rc = _coarse(17, q_lens, r_lens)
    qf, rf = _att_inputs(50, q_lens, regions, dim), _att_inputs(51, r_lens, regions, dim)
    c = HalfCtx(qc, rc)

    def run(qx, rx):
        qd, rd = dec(qx), dec(rx)
        for symmetric in (True, False):
            _same_bits(pairs, c.stage1(pairs, symmetric), [ref.fine_sim(qd[q], rd[r], "att", symmetric) for q, r in pairs], symmetric)

    def spoiled(fine, value, as_half_bits=False):
        """A copy with the LAST element of the side replaced (fp32 value, or the bits of a half)."""
        out = [x.astype(F16) if as_half_bits else x.copy() for x in fine]
        if as_half_bits:
            out[-1].view(np.uint16)[-1, -1, -1] = value
        else:
            out[-1][-1, -1, -1] = value
        return out

    def refused(side, fine, src_f16):
        rc_ = c.set_fine_f16(fine if side == "query" else None, fine if side == "reference" else None, src_f16, check=False)
        msg = c.L.vsc_last_error().decode()
        assert rc_ == _lib.VSC_ERR_INVALID and msg.startswith("vsc_tn_set_fine_f16: a %s fine descriptor" % side), (rc_, msg)
        other = r_lens if side == "query" else q_lens
        assert c.fine_bytes() == _side_bytes(sum(other), regions, dim)  # the written side holds nothing
        _refuses(c, pairs, side)

    try:
        c.set_fine_f16(qf, rf, 0)
        run(qf, rf)
        with np.errstate(all="ignore"):
            for value in (np.inf, -np.inf, np.nan, 65536.0, -65536.0):
                refused("query", spoiled(qf, value), 0)
                c.set_fine_f16(qf, None, 0)  # the reference side was untouched: stage 1 is right again
                run(qf, rf)
            for bits in (0x7C00, 0xFC00, 0x7E00):  # +inf, -inf, a quiet NaN as halves
                refused("reference", spoiled(rf, bits, as_half_bits=True), 1)
                c.set_fine_f16(None, rf, 1)
                run(qf, rf)
            # both sides in one call, the second one spoiled: the first is stored, the second is gone
            qf2 = _att_inputs(52, q_lens, regions, dim)
            assert c.set_fine_f16(qf2, spoiled(rf, np.nan), 0, check=False) == _lib.VSC_ERR_INVALID
            assert c.L.vsc_last_error().decode().startswith("vsc_tn_set_fine_f16: a reference fine descriptor")
            assert c.fine_bytes() == _side_bytes(sum(q_lens), regions, dim)
            _refuses(c, pairs, "reference")
            c.set_fine_f16(None, rf, 0)
            assert c.L.vsc_tn_set_fine_f16(c.ctx, None, None, regions, dim, 0, _lib.MEM_HOST) == 0  # (nothing to do)
            run(qf2, rf)
            # the largest half is no refusal
            top_q, top_r = spoiled(qf, 65504.0), spoiled(rf, -65504.0)
            c.set_fine_f16(top_q, top_r, 0)
            run(top_q, top_r)
        # as ValueError through the library's error mapping
        with pytest.raises(ValueError, match="beyond \\+-65504"):
            c.set_fine_f16(spoiled(qf, 1e9), None, 0)
        c.set_fine_f16(qf, None, 1)
        run(qf, top_r)
    finally:
        c.close()


def test_refusals(gpu, orc):
    _refusal_sequence()


# ---- 5. device-resident sources -------------------------------------------------------------------------------------

def test_device_sources_equal_host_sources(gpu):
    regions, dim = 9, 72
    q_lens, r_lens = tile_lens(regions)
    pairs = all_pairs(q_lens, r_lens)
    qc, rc = _coarse(18, q_lens, r_lens)
    qf, rf = _att_inputs(60, q_lens, regions, dim), _att_inputs(61, r_lens, regions, dim)
    qh, rh = [x.astype(F16) for x in qf], [x.astype(F16) for x in rf]
    c = HalfCtx(qc, rc)
    try:
        c.set_fine_f16(qf, rf, 0)
        want = {s: c.stage1(pairs, s) for s in (False, True)}
        for src_f16, (qx, rx) in ((0, (qf, rf)), (1, (qh, rh))):
            c.set_fine(qf, rf, "att")  # (another store in between: both sides are rewritten below)
            c.set_fine_f16(qx, rx, src_f16, device=True)
            for s in (False, True):
                _same_bits(pairs, c.stage1(pairs, s), want[s], src_f16, s)
        c.set_fine_f16(qh, None, 1, device=True)  # one side from the device, the other kept
        _same_bits(pairs, c.stage1(pairs, True), want[True])
    finally:
        c.close()


# ---- 6. the public route --------------------------------------------------------------------------------------------

def _public_case(qfine, rfine, fine_codec, **kw):
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity, VCSLLocalizationDnS
    from vsc2022_amd.vsc.metrics import CandidatePair

    qc, rc, _, _ = _public_inputs()
    (qv, qfv), (rv, rfv) = ref.video_features(qc, qfine, "Q"), ref.video_features(rc, rfine, "R")
    loc = VCSLLocalizationDnS(ChamferSimilarity("att"), qfv, rfv, qv, rv, model_type="TN", tn_max_step=5, min_length=4,
                              concurrency=16, similarity_bias=0.5, device="cpu", on_device=True, fine_codec=fine_codec, **kw)
    cands = [CandidatePair(qv[q].video_id, rv[r].video_id, 1.0 - 0.01 * k) for k, (q, r) in enumerate(ref.CLASS_PAIRS)]
    return loc, cands


_PUBLIC = {}


def _public_inputs():
    if "in" not in _PUBLIC:
        _PUBLIC["in"] = ref.class_inputs("att")
    return _PUBLIC["in"]


def _public_fine(symmetric):
    """F of every class pair on the half-rounded descriptors, computed once per value of `symmetric`."""
    key = ("fine", bool(symmetric))
    if key not in _PUBLIC:
        _, _, qf, rf = _public_inputs()
        qd, rd = dec(qf), dec(rf)
        _PUBLIC[key] = [ref.fine_sim(qd[q], rd[r], "att", bool(symmetric)) for q, r in ref.CLASS_PAIRS]
    return _PUBLIC[key]


def _equal_routes(a, b, cands):
    from vsc2022_amd.vsc.metrics import Match

    got, want = a.localize_all(cands), b.localize_all(cands)
    assert len(want) >= 5 and got == want
    assert np.array_equal(helpers.bits(np.array([m.score for m in got], dtype=F32)), helpers.bits(np.array([m.score for m in want], dtype=F32)))
    ta, tb = a.localize_table(cands), b.localize_table(cands)
    assert ta.to_matches() == got
    for field in Match._fields + ("pair", "boxes"):
        x, y = getattr(ta, field), getattr(tb, field)
        assert x.dtype == y.dtype and np.array_equal(x, y), field
    for c in cands:
        assert np.array_equal(helpers.bits(a.similarity(c)), helpers.bits(b.similarity(c)))
    return got


@pytest.mark.parametrize("geometric_mean,symmetric", [(1, 1), (0, 1), (1, 0)])
def test_public_route_on_half_features(gpu, orc, geometric_mean, symmetric):
    """float16 features (what dns_index writes): the half store == the default store on the same features == the CPU
    chain fine_sim -> blend -> localise with the reference's parameters."""
    qc, rc, qf, rf = _public_inputs()
    qh, rh = [x.astype(F16) for x in qf], [x.astype(F16) for x in rf]
    kw = dict(geometric_mean=bool(geometric_mean), symmetric=bool(symmetric))
    half, cands = _public_case(qh, rh, "SQfp16", **kw)
    plain, _ = _public_case(qh, rh, None, **kw)
    assert 0 < half.fine_bytes and half.fine_bytes * 2 == plain.fine_bytes
    got = _equal_routes(half, plain, cands)
    want = []
    for c, (q, r), fine in zip(cands, ref.CLASS_PAIRS, _public_fine(symmetric)):
        s = ref.blend(fine, orc.pair_sims(qc[q], rc[r], 0.5)) if geometric_mean else fine
        assert np.array_equal(helpers.bits(half.similarity(c)), helpers.bits(s))
        boxes, scores = ref.localise(s, ref.REF_PARAMS, 0.5)
        want += [(c.query_id, c.ref_id, float(x1), float(x2 + 1), float(y1), float(y2 + 1), sc) for (x1, y1, x2, y2), sc in zip(boxes, scores)]
    assert len(want) >= 5
    assert [(m.query_id, m.ref_id, m.query_start, m.query_end, m.ref_start, m.ref_end) for m in got] == [w[:6] for w in want]
    assert np.array_equal(helpers.bits(np.array([m.score for m in got])), helpers.bits(np.array([w[6] for w in want])))


def test_public_route_rounds_fp32_features(gpu):
    """float32 features that no half holds: the results of the default store on half_rounded features."""
    _, _, qf, rf = _public_inputs()
    assert all(x.dtype == F32 for x in qf + rf) and any((ref.half_rounded(x) != x).any() for x in qf)
    half, cands = _public_case(qf, rf, "SQfp16")
    plain, _ = _public_case(dec(qf), dec(rf), None)
    assert half.fine_bytes * 2 == plain.fine_bytes
    _equal_routes(half, plain, cands)


def test_public_route_refuses_what_a_half_cannot_hold(gpu):
    _, _, qf, rf = _public_inputs()
    bad = [x.copy() for x in qf]
    bad[2][3, 1, 5] = 1e6
    with pytest.raises(ValueError, match="beyond \\+-65504"):
        _public_case(bad, rf, "SQfp16")


# ---- 7. poisoned allocations ----------------------------------------------------------------------------------------

def _poison_sequence():
    """The smallest case of 1, then the sequence of 4, on fresh handles."""
    import oracle as orc

    orc.build()
    regions, dim = 1, 1
    q_lens, r_lens = tile_lens(regions)
    qc, rc = _coarse(11, q_lens, r_lens)
    c = HalfCtx(qc, rc)
    try:
        _four_ways(c, _att_inputs(1001, q_lens, regions, dim), _att_inputs(1002, r_lens, regions, dim), all_pairs(q_lens, r_lens))
    finally:
        c.close()
    _refusal_sequence()


def test_with_poisoned_allocations(gpu):
    """Under VSC_POISON_ALLOC=1 in a fresh process every new device buffer starts as 0xFF bytes -- NaN halves, which a
    slack row or a k padding that nobody zeroed would carry into the chain."""
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_fine_f16 as t; t._poison_sequence(); print('poison ok')" % (
        ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, VSC_POISON_ALLOC="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
