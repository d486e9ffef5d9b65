"""The 1-bit store of DnS's binary fine descriptors on the device (vsc_tn_set_fine_bits, fine_bits.hip) against the CPU
restatement in tests/dns_fine_ref.py and against the +-1 fp32 store of the same descriptors: BIT PATTERNS throughout --
the integer kernel has a proof (include/vscmi.h; tests/test_fine_bits_host.py checks it on the CPU), not a tolerance.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dns_fine_ref as ref
import helpers
from test_gpu_dns_device import S1_PAIRS, S1_PAIRS_WIDE, S1_Q_LENS, S1_R_LENS, Ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def packed_rows(fine, garbage=False):
    """np.packbits rows of a list of videos; garbage: the unused high bits of the last byte set in every other row (in
    all rows they would cancel in the xor of two rows whether or not the library masks them)."""
    x = np.ascontiguousarray(np.packbits(np.concatenate(fine, axis=0), axis=-1, bitorder="little"))
    tail = fine[0].shape[2] % 8
    if garbage and tail:
        x.reshape(-1, x.shape[-1])[0::2, -1] |= np.uint8((0xFF << tail) & 0xFF)
    return x


class BitsCtx(Ctx):
    def set_fine_bits(self, qf, rf, packed, check=True, garbage=False, device=False):
        def rows(fine):
            if fine is None:
                return None
            if packed:
                return packed_rows(fine, garbage)
            return np.ascontiguousarray(np.concatenate(fine, axis=0), dtype=np.uint8)

        some = next(f for f in (qf or rf) if f is not None)
        q, r = rows(qf), rows(rf)
        mem, keep = self._lib.MEM_HOST, []
        addr = [None if x is None else x.ctypes.data for x in (q, r)]
        if device:
            import torch

            keep = [None if x is None else torch.from_numpy(x).to("cuda:0") for x in (q, r)]
            torch.cuda.synchronize()
            addr, mem = [None if t is None else t.data_ptr() for t in keep], self._lib.MEM_DEVICE
        rc = self.L.vsc_tn_set_fine_bits(self.ctx, addr[0], addr[1], some.shape[1], some.shape[2], int(packed), mem)
        if check:
            self._lib.check(rc)
        return rc

    def fine_bytes(self):
        return int(self.L.vsc_tn_fine_bytes(self.ctx))


def _bin_inputs(seed, lens, regions, dim):
    rng = np.random.default_rng(seed)
    return [rng.random((n, regions, dim)) > 0.5 for n in lens]


def _coarse(seed, q_lens, r_lens):
    rng = np.random.default_rng(seed)
    return [ref.unit_rows(rng, n, 16) for n in q_lens], [ref.unit_rows(rng, n, 16) for n in r_lens]


def _same_bits(pairs, got, want, *what):
    for p, a, b in zip(pairs, got, want):
        assert a.shape == b.shape and np.array_equal(helpers.bits(a), helpers.bits(b)), (p,) + what


# ---- 1. stage 1 is the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("regions,dim", [(1, 1), (1, 16), (4, 20), (9, 33), (16, 31), (4, 65), (16, 64), (1, 64), (9, 512), (4, 512)])
def test_stage1_is_the_restatement(gpu, orc, regions, dim):
    """The frame counts of test_gpu_dns_device.py (tile edges of every R, a video without frames); widths on both sides
    of the 8-, 32- and 64-bit boundaries; both input forms, `symmetric` both ways, host and device output."""
    qc, rc = _coarse(7, S1_Q_LENS, S1_R_LENS)
    qf = _bin_inputs(regions * 1000 + dim, S1_Q_LENS, regions, dim)
    rf = _bin_inputs(regions * 1000 + dim + 1, S1_R_LENS, regions, dim)
    pairs = S1_PAIRS_WIDE if dim == 512 else S1_PAIRS
    g = {p: ref.region_matrix(qf[p[0]], rf[p[1]], "bin") for p in set(pairs) if S1_Q_LENS[p[0]] and S1_R_LENS[p[1]]}
    want = {s: [ref.fine_sim(qf[q], rf[r], "bin", s, g.get((q, r))) for q, r in pairs] for s in (False, True)}
    c = BitsCtx(qc, rc)
    try:
        for packed in (0, 1):
            c.set_fine_bits(qf, rf, packed, garbage=True)
            for symmetric in (False, True):
                for device_out in (False, True):
                    rc_, got, _ = c.fine_similarity(pairs, symmetric, device_out=device_out)
                    assert rc_ == 0, c.L.vsc_last_error()
                    _same_bits(pairs, got, want[symmetric], packed, symmetric, device_out)
    finally:
        c.close()


# ---- 2. equal to the fp32 BIN store ---------------------------------------------------------------------------------

@pytest.mark.parametrize("regions,dim", [(9, 512), (4, 65), (16, 31), (1, 129)])
def test_equal_to_the_fp32_bin_store(gpu, regions, dim):
    """One context, the same descriptors through vsc_tn_set_fine(BIN) and through vsc_tn_set_fine_bits (host and device
    sources): every pair of the long list, no oracle in between."""
    qc, rc = _coarse(9, S1_Q_LENS, S1_R_LENS)
    qf = _bin_inputs(regions * 77 + dim, S1_Q_LENS, regions, dim)
    rf = _bin_inputs(regions * 77 + dim + 1, S1_R_LENS, regions, dim)
    c = BitsCtx(qc, rc)
    try:
        c.set_fine(qf, rf, "bin")
        by_bin = {}
        for symmetric in (False, True):
            rc_, by_bin[symmetric], _ = c.fine_similarity(S1_PAIRS, symmetric)
            assert rc_ == 0, c.L.vsc_last_error()
        for packed, device in ((1, False), (0, True), (1, True)):
            c.set_fine_bits(qf, rf, packed, device=device)
            for symmetric in (False, True):
                rc_, got, _ = c.fine_similarity(S1_PAIRS, symmetric, device_out=True)
                assert rc_ == 0, c.L.vsc_last_error()
                _same_bits(S1_PAIRS, got, by_bin[symmetric], packed, device, symmetric)
    finally:
        c.close()


# ---- 3. extremes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [33, 65, 127, 513])
def test_extremes(gpu, orc, dim):
    """What a counted pad bit or a lost word would move: all-ones against all-zeros (every G = -1: F = 0.0 exactly),
    identical rows (F = 1.0), and single differing bits at the last valid position and at the first position of the last
    8-, 32-, 64- and 128-bit word of a row.  Garbage in the packed input's tail bits changes nothing."""
    regions, q_lens, r_lens = 3, (5, 8, 8, 8), (6, 7, 7, 7)
    rng = np.random.default_rng(dim)
    base = rng.random(dim) > 0.5
    spots = sorted({dim - 1} | {w * ((dim - 1) // w) for w in (8, 32, 64, 128)})
    qf = [np.ones((5, regions, dim), bool)] + [np.broadcast_to(base, (8, regions, dim)).copy() for _ in range(3)]
    rf = [np.zeros((6, regions, dim), bool)] + [np.broadcast_to(base, (7, regions, dim)).copy() for _ in range(3)]
    rf[2][..., dim - 1] ^= True                      # the last valid position, every row
    for k, d in enumerate(spots):                    # one spot per (frame, region) in turn, one bit per row
        rf[3].reshape(-1, dim)[k::len(spots), d] ^= True
    pairs = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (1, 0)]
    qc, rc = _coarse(3, q_lens, r_lens)
    c = BitsCtx(qc, rc)
    try:
        for symmetric in (False, True):
            want = [ref.fine_sim(qf[q], rf[r], "bin", symmetric) for q, r in pairs]
            assert (want[0] == 0.0).all() and (want[1] == 1.0).all()
            for k in (2, 3):  # one bit of D apart: below 1, and the same value wherever the bit sits
                assert (want[k] < 1.0).all() and (want[k] == want[2][0, 0]).all()
            for packed, garbage in ((0, False), (1, False), (1, True)):
                c.set_fine_bits(qf, rf, packed, garbage=garbage)
                rc_, got, _ = c.fine_similarity(pairs, symmetric)
                assert rc_ == 0, c.L.vsc_last_error()
                assert not np.signbit(got[0]).any()
                _same_bits(pairs, got, want, packed, garbage, symmetric)
    finally:
        c.close()


# ---- 4. memory ------------------------------------------------------------------------------------------------------

def test_memory(gpu):
    regions, dim = 9, 512
    qc, rc = _coarse(4, S1_Q_LENS, S1_R_LENS)
    qf, rf = _bin_inputs(40, S1_Q_LENS, regions, dim), _bin_inputs(41, S1_R_LENS, regions, dim)
    rows = (sum(S1_Q_LENS) + sum(S1_R_LENS)) * regions
    c = BitsCtx(qc, rc)
    try:
        c.set_fine(qf, rf, "bin")
        as_fp32 = c.fine_bytes()
        assert as_fp32 >= rows * dim * 4
        c.set_fine_bits(qf, rf, 1)
        as_bits = c.fine_bytes()
        assert as_bits * 16 <= as_fp32  # (32 in the limit; the factor 2 covers the slack rows and the padding choice)
        assert as_bits >= rows * ((dim + 7) // 8)
        c.set_fine_bits(qf, None, 0)  # one side again: the counter is per side, not cumulative
        assert c.fine_bytes() == as_bits
    finally:
        c.close()


# ---- 5. handle reuse ------------------------------------------------------------------------------------------------

def _reuse_sequence():
    """One context through BIN -> BITS -> ATT -> BITS with different (regions, fdim), stage 1 against the restatement
    after each; a NULL side keeps what it had; a new query side drops the query bits; refused arguments leave a context
    that still works."""
    import oracle as orc
    from vsc2022_amd import _lib

    orc.build()
    q_lens, r_lens = (7, 8, 20, 0, 33), (9, 31, 1, 16)
    pairs = [(0, 0), (1, 1), (2, 2), (4, 1), (3, 0), (2, 3), (4, 3), (0, 2)]
    qc, rc = _coarse(50, q_lens, r_lens)
    c = BitsCtx(qc, rc)

    def run(qf, rf, kind):
        for symmetric in (True, False):
            rc_, got, _ = c.fine_similarity(pairs, symmetric, device_out=True)
            assert rc_ == 0, c.L.vsc_last_error()
            _same_bits(pairs, got, [ref.fine_sim(qf[q], rf[r], kind, symmetric) for q, r in pairs], kind, symmetric)

    def att(seed, lens, regions, dim):
        rng = np.random.default_rng(seed)
        return [ref.unit_rows(rng, n * regions, dim).reshape(n, regions, dim) for n in lens]

    try:
        qf, rf = _bin_inputs(51, q_lens, 9, 70), _bin_inputs(52, r_lens, 9, 70)
        c.set_fine(qf, rf, "bin")
        run(qf, rf, "bin")
        qf, rf = _bin_inputs(53, q_lens, 4, 33), _bin_inputs(54, r_lens, 4, 33)
        c.set_fine_bits(qf, None, 0)  # (another shape and store: both sides were dropped, one is back)
        rc_ = c.fine_similarity(pairs, True)[0]
        assert rc_ == _lib.VSC_ERR_INVALID and b"no reference fine descriptors" in c.L.vsc_last_error()
        c.set_fine_bits(None, rf, 1)
        run(qf, rf, "bin")
        qa, ra = att(55, q_lens, 4, 33), att(56, r_lens, 4, 33)
        c.set_fine(qa, None, "att")  # (the same shape, another store: the bit rows of the reference side are gone)
        assert c.fine_similarity(pairs, True)[0] == _lib.VSC_ERR_INVALID
        c.set_fine(None, ra, "att")
        run(qa, ra, "att")
        qf, rf = _bin_inputs(57, q_lens, 16, 200), _bin_inputs(58, r_lens, 16, 200)
        c.set_fine_bits(qf, rf, 1, garbage=True)
        run(qf, rf, "bin")
        rf2 = _bin_inputs(59, r_lens, 16, 200)
        c.set_fine_bits(None, rf2, 0)  # a NULL side keeps what it had
        run(qf, rf2, "bin")
        # refused arguments: the context is as it was
        x = np.zeros(64, np.uint8)
        for regions, dim, packed in ((16, (1 << 24) + 1, 1), (16, 200, 2), (17, 200, 0), (0, 200, 0), (16, 0, 1), (16, 200, -1)):
            assert c.L.vsc_tn_set_fine_bits(c.ctx, x.ctypes.data, None, regions, dim, packed, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID
            assert c.L.vsc_last_error().decode() == "vsc_tn_set_fine_bits: invalid argument (regions 1..16, fdim 1..16777216, packed 0 / 1)"
        assert c.L.vsc_tn_set_fine(c.ctx, x.ctypes.data, None, 16, 200, _lib.FINE_BITS, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID
        run(qf, rf2, "bin")
        # a new query side drops the query bits
        q_lens2 = (12, 0, 8, 9, 30)
        qc2, _ = _coarse(60, q_lens2, r_lens)
        c.set_queries(qc2)
        rc_ = c.fine_similarity(pairs, True)[0]
        assert rc_ == _lib.VSC_ERR_INVALID and b"no query fine descriptors" in c.L.vsc_last_error()
        qf2 = _bin_inputs(61, q_lens2, 16, 200)
        c.set_fine_bits(qf2, None, 1)
        pairs[:] = [(0, 0), (2, 1), (4, 3), (1, 2), (3, 3)]
        run(qf2, rf2, "bin")
    finally:
        c.close()


def test_handle_reuse(gpu, orc):
    _reuse_sequence()


def test_handle_reuse_with_poisoned_allocations(gpu):
    """The same sequence under VSC_POISON_ALLOC=1 in a fresh process: every new device buffer starts as 0xFF bytes, which
    a slack row or a K padding that nobody zeroed would carry into a popcount."""
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_fine_bits as t; t._reuse_sequence(); print('reuse ok')" % (
        ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, VSC_POISON_ALLOC="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "reuse ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- 6. the public route --------------------------------------------------------------------------------------------

def _g9_case(fine_codec, as_uint8=False):
    from vsc2022_amd import synth
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity, VCSLLocalizationDnS
    from vsc2022_amd.vsc.index import VideoFeature
    from vsc2022_amd.vsc.metrics import CandidatePair

    fx = helpers.load("g9_dns_bin")
    fg_type = str(fx["fg_type"])
    q, r, qfine, rfine = helpers.g9_inputs(fg_type)
    if as_uint8:
        qfine, rfine = [f.astype(np.uint8) for f in qfine], [f.astype(np.uint8) for f in rfine]
    qc, rc = synth.to_video_features(q, VideoFeature), synth.to_video_features(r, VideoFeature)
    qf = {v.video_id: VideoFeature(video_id=v.video_id, timestamps=v.timestamps, feature=f) for v, f in zip(qc, qfine)}
    rf = {v.video_id: VideoFeature(video_id=v.video_id, timestamps=v.timestamps, feature=f) for v, f in zip(rc, rfine)}
    loc = VCSLLocalizationDnS(ChamferSimilarity(fg_type), qf, rf, qc, rc, model_type="TN", tn_max_step=5, min_length=4,
                              concurrency=16, similarity_bias=0.5, device="cpu", symmetric=bool(fx["symmetric"]),
                              geometric_mean=bool(fx["geometric_mean"]), on_device=True, fine_codec=fine_codec)
    cands = [CandidatePair(str(a), str(b), float(s)) for a, b, s in zip(fx["cand_q"], fx["cand_r"], fx["cand_s"])]
    return fx, loc, cands


def test_public_route_equals_the_default_store(gpu):
    from vsc2022_amd.vsc.metrics import Match

    fx, bits, cands = _g9_case("bits")
    _, plain, _ = _g9_case(None)
    _, from_bytes, _ = _g9_case("bits", as_uint8=True)
    assert 0 < bits.fine_bytes < plain.fine_bytes and from_bytes.fine_bytes == bits.fine_bytes
    want = plain.localize_all(cands)
    got = bits.localize_all(cands)
    assert len(want) >= 5 and len(got) == len(want)
    for a, b in zip(got, want):  # match for match; the scores as bits
        assert a._replace(score=0.0) == b._replace(score=0.0)
        assert np.array_equal(helpers.bits(a.score), helpers.bits(b.score))
    assert from_bytes.localize_all(cands) == got
    ta, tb = bits.localize_table(cands), plain.localize_table(cands)
    assert ta.to_matches() == got
    for field in Match._fields + ("pair", "boxes"):
        x, y = getattr(ta, field), getattr(tb, field)
        assert x.dtype == y.dtype and np.array_equal(x, y), field
    for c in cands:
        assert np.array_equal(helpers.bits(bits.similarity(c)), helpers.bits(plain.similarity(c)))
    # the reference's golden, under the conditions of test_class_with_chamfer_on_the_reference_goldens
    cuts = np.r_[0, np.cumsum(fx["sim_shapes"].prod(axis=1))]
    for k in range(0, len(cands), 5):
        sim_want = fx["sims"][cuts[k]:cuts[k + 1]].reshape(fx["sim_shapes"][k])
        sim_got = bits.similarity(cands[k])
        assert sim_got.shape == sim_want.shape and np.abs(sim_got - sim_want).max() < 2e-6, (k, np.abs(sim_got - sim_want).max())
    rows = fx["m_rows"]
    assert len(got) == len(rows)
    assert [str(m.query_id) for m in got] == list(fx["m_q"]) and [str(m.ref_id) for m in got] == list(fx["m_r"])
    arr = np.array([[m.score, m.query_start, m.query_end, m.ref_start, m.ref_end] for m in got], dtype=np.float64)
    assert np.array_equal(arr[:, 1:], rows[:, 1:])
    assert np.abs(arr[:, 0] - rows[:, 0]).max() < 4e-6
