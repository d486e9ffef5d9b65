"""DnS localisation on the device against the CPU restatement in tests/dns_fine_ref.py: the region Chamfer kernel
(vsc_tn_fine_similarity), the blend inside the Temporal-Network kernel (vsc_tn_localize_fine, vsc_tn_similarity_fine)
and `VCSLLocalizationDnS(on_device=True)` -- bits wherever the arithmetic is the engine's own.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dns_fine_ref as ref
import helpers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


class Ctx:
    """A localisation context over lists of coarse videos, with the raw calls the tests need."""

    def __init__(self, qc, rc, codec="Flat"):
        from vsc2022_amd import _lib

        self.L, self._lib = _lib.lib(), _lib
        self.q_lens, self.r_lens = [len(v) for v in qc], [len(v) for v in rc]
        self.dim = qc[0].shape[1]
        self.ctx = ctypes.c_void_p()
        q_rows, q_off = self._rows(qc)
        r_rows, r_off = self._rows(rc)
        _lib.check(self.L.vsc_tn_create_codec(q_rows.ctypes.data, q_off.ctypes.data, len(qc), r_rows.ctypes.data, 0,
                                              r_off.ctypes.data, len(rc), self.dim, _lib.MEM_HOST, _lib.MEM_HOST,
                                              _lib.codec_id(codec), 0, ctypes.byref(self.ctx)))

    def _rows(self, videos):
        rows = np.ascontiguousarray(np.concatenate(videos, axis=0), dtype=F32)
        return rows, np.r_[0, np.cumsum([len(v) for v in videos])].astype(np.int64)

    def close(self):
        self.L.vsc_tn_destroy(self.ctx)

    def set_queries(self, qc):
        rows, off = self._rows(qc)
        self.q_lens = [len(v) for v in qc]
        self._lib.check(self.L.vsc_tn_set_queries(self.ctx, rows.ctypes.data, off.ctypes.data, len(qc), self._lib.MEM_HOST))

    def set_fine(self, qf, rf, kind, check=True):
        def rows(fine):
            if fine is None:
                return None
            x = np.concatenate(fine, axis=0)
            return np.ascontiguousarray(x, dtype=np.uint8 if kind == "bin" else F32)

        some = next(f for f in (qf or rf) if f is not None)
        q, r = rows(qf), rows(rf)
        rc = self.L.vsc_tn_set_fine(self.ctx, None if q is None else q.ctypes.data, None if r is None else r.ctypes.data,
                                    some.shape[1], some.shape[2], self._lib.FINE_BIN if kind == "bin" else self._lib.FINE_ATT,
                                    self._lib.MEM_HOST)
        if check:
            self._lib.check(rc)
        return rc

    def offsets(self, pairs):
        cells = np.array([self.q_lens[q] * self.r_lens[r] for q, r in pairs], dtype=np.int64)
        return np.r_[0, np.cumsum(cells)[:-1]].astype(np.int64), cells

    def fine_similarity(self, pairs, symmetric, device_out=False, cap=None):
        """(rc, list of F matrices); the output is pre-filled with a canary."""
        pq, pr = (np.array(x, dtype=np.int32) for x in zip(*pairs))
        off, cells = self.offsets(pairs)
        total = int(cells.sum())
        cap = total if cap is None else cap
        if device_out:
            import torch

            out_t = torch.full((max(total, 1),), -7.25, dtype=torch.float32, device="cuda:0")
            off_t = torch.from_numpy(off).to("cuda:0")
            torch.cuda.synchronize()
            rc = self.L.vsc_tn_fine_similarity(self.ctx, pq.ctypes.data, pr.ctypes.data, len(pairs), self._lib.MEM_HOST,
                                               int(symmetric), out_t.data_ptr(), off_t.data_ptr(), cap, self._lib.MEM_DEVICE)
            out = out_t.cpu().numpy()
        else:
            out = np.full(max(total, 1), -7.25, dtype=F32)
            rc = self.L.vsc_tn_fine_similarity(self.ctx, pq.ctypes.data, pr.ctypes.data, len(pairs), self._lib.MEM_HOST,
                                               int(symmetric), out.ctypes.data, off.ctypes.data, cap, self._lib.MEM_HOST)
        mats = [out[o:o + c].reshape(self.q_lens[q], self.r_lens[r]) for (q, r), o, c in zip(pairs, off, cells)]
        return rc, mats, out

    def localize_fine(self, pairs, mats, geometric_mean, params, bias, device_slab=False):
        from vsc2022_amd.vcsl.vta import build_vta_model

        prm = build_vta_model("TN", **params).params
        pq, pr = (np.array(x, dtype=np.int32) for x in zip(*pairs))
        off, cells = self.offsets(pairs)
        slab = np.concatenate([np.ascontiguousarray(m, dtype=F32).ravel() for m in mats] + [np.zeros(1, dtype=F32)])
        n = len(pairs)
        n_boxes = np.full(n, -1, dtype=np.int32)
        boxes = np.zeros((n, self._lib.TN_MAX_BOXES, 4), dtype=np.int32)
        box_max = np.zeros((n, self._lib.TN_MAX_BOXES), dtype=F32)
        if device_slab:
            import torch

            keep = (torch.from_numpy(slab).to("cuda:0"), torch.from_numpy(off).to("cuda:0"))
            torch.cuda.synchronize()
            fine, fine_off, mem = keep[0].data_ptr(), keep[1].data_ptr(), self._lib.MEM_DEVICE
        else:
            fine, fine_off, mem = slab.ctypes.data, off.ctypes.data, self._lib.MEM_HOST
        self._lib.check(self.L.vsc_tn_localize_fine(
            self.ctx, pq.ctypes.data, pr.ctypes.data, n, self._lib.MEM_HOST, fine, fine_off, mem, int(geometric_mean),
            ctypes.byref(prm), float(bias), n_boxes.ctypes.data, boxes.ctypes.data, box_max.ctypes.data, self._lib.MEM_HOST))
        return n_boxes, boxes, box_max

    def similarity_fine(self, q, r, bias, fine, geometric_mean):
        out = np.full((self.q_lens[q], self.r_lens[r]), -7.25, dtype=F32)
        fine = np.ascontiguousarray(fine, dtype=F32)
        self._lib.check(self.L.vsc_tn_similarity_fine(self.ctx, q, r, float(bias), fine.ctypes.data, self._lib.MEM_HOST,
                                                      int(geometric_mean), out.ctypes.data, out.size, None, None))
        return out


# ---- 1. stage 1 bits ------------------------------------------------------------------------------------------------

# frame counts around the tile edge of every R (64 / R frames per tile: 64, 16, 7, 4), a video without frames, and a
# pair list that repeats videos and mixes the longest with the shortest
S1_Q_LENS = (1, 6, 7, 8, 31, 32, 33, 64, 65, 100, 0)
S1_R_LENS = (100, 65, 64, 33, 32, 31, 8, 7, 6, 1, 0)
S1_PAIRS = [(k, k) for k in range(11)] + [(k, (k + 3) % 11) for k in range(11)] + [(9, 0), (9, 0), (0, 9), (10, 0), (9, 10), (7, 2)]
# at D = 512 the oracle's chains cost: the longest videos meet there once
S1_PAIRS_WIDE = [(k, 9 - k) for k in range(10)] + [(5, 5), (5, 5), (10, 3), (3, 10), (8, 2), (9, 1)]


def _fine_inputs(seed, lens, regions, dim, kind):
    rng = np.random.default_rng(seed)
    if kind == "bin":
        return [rng.random((n, regions, dim)) > 0.5 for n in lens]
    return [ref.unit_rows(rng, n * regions, dim).reshape(n, regions, dim) for n in lens]


@pytest.mark.parametrize("kind", ["att", "bin"])
@pytest.mark.parametrize("regions,dim", [(1, 16), (4, 20), (9, 512), (16, 64), (9, 20), (16, 16), (1, 64), (4, 512)])
def test_stage1_is_the_restatement(gpu, orc, regions, dim, kind):
    rng = np.random.default_rng(7)
    qc = [ref.unit_rows(rng, n, 16) for n in S1_Q_LENS]
    rc = [ref.unit_rows(rng, n, 16) for n in S1_R_LENS]
    qf = _fine_inputs(regions * 1000 + dim, S1_Q_LENS, regions, dim, kind)
    rf = _fine_inputs(regions * 1000 + dim + 1, S1_R_LENS, regions, dim, kind)
    pairs = S1_PAIRS_WIDE if dim == 512 else S1_PAIRS
    c = Ctx(qc, rc)
    try:
        c.set_fine(qf, rf, kind)
        rows = sum(S1_Q_LENS) * regions, sum(S1_R_LENS) * regions
        assert c.L.vsc_tn_fine_bytes(c.ctx) >= (rows[0] + rows[1]) * dim * 4
        g = {p: ref.region_matrix(qf[p[0]], rf[p[1]], kind) for p in set(pairs) if S1_Q_LENS[p[0]] and S1_R_LENS[p[1]]}
        for symmetric in (False, True):
            want = [ref.fine_sim(qf[q], rf[r], kind, symmetric, g.get((q, r))) for q, r in pairs]
            for device_out in (False, True):
                rc_, got, _ = c.fine_similarity(pairs, symmetric, device_out=device_out)
                assert rc_ == 0, c.L.vsc_last_error()
                for p, a, b in zip(pairs, got, want):
                    assert np.array_equal(helpers.bits(a), helpers.bits(b)), (p, symmetric, device_out, np.abs(a - b).max())
    finally:
        c.close()


def test_stage1_arguments(gpu, orc):
    from vsc2022_amd import _lib

    rng = np.random.default_rng(8)
    qc, rc = [ref.unit_rows(rng, n, 16) for n in (5, 9)], [ref.unit_rows(rng, n, 16) for n in (8, 3)]
    qf, rf = _fine_inputs(1, (5, 9), 4, 16, "att"), _fine_inputs(2, (8, 3), 4, 16, "att")
    c = Ctx(qc, rc)
    try:
        pairs = [(0, 0), (1, 1)]
        assert c.fine_similarity(pairs, True)[0] == _lib.VSC_ERR_INVALID  # no fine descriptors yet
        for regions, dim, kind in ((0, 16, 0), (17, 16, 0), (4, 0, 0), (4, 16, 2)):
            x = np.zeros((14, max(regions, 1), max(dim, 1)), dtype=F32)
            assert c.L.vsc_tn_set_fine(c.ctx, x.ctypes.data, None, regions, dim, kind, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID
        c.set_fine(qf, None, "att")
        assert c.fine_similarity(pairs, True)[0] == _lib.VSC_ERR_INVALID  # the reference side is still missing
        c.set_fine(None, rf, "att")
        rc_, got, _ = c.fine_similarity(pairs, True)
        assert rc_ == 0 and np.array_equal(helpers.bits(got[1]), helpers.bits(ref.fine_sim(qf[1], rf[1], "att", True)))
        rc_, _, out = c.fine_similarity(pairs, True, cap=5 * 8 + 9 * 3 - 1)
        assert rc_ == _lib.VSC_ERR_CAPACITY and (out == F32(-7.25)).all()  # nothing written
        pq, pr = np.array([0, 2], dtype=np.int32), np.array([0, 0], dtype=np.int32)
        off, out = np.array([0, 40], dtype=np.int64), np.zeros(200, dtype=F32)
        assert c.L.vsc_tn_fine_similarity(c.ctx, pq.ctypes.data, pr.ctypes.data, 2, _lib.MEM_HOST, 1, out.ctypes.data,
                                          off.ctypes.data, 200, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID  # ordinal out of range
    finally:
        c.close()


def test_failed_upload_of_another_shape_keeps_no_side(gpu, orc):
    """A store of another kind or shape drops both sides before the first upload: when the query side is then refused, the
    reference side of the old store is gone too, though its own upload was never reached.  (The new rows are no larger
    than the old ones.)"""
    from vsc2022_amd import _lib

    rng = np.random.default_rng(9)
    qc, rc = [ref.unit_rows(rng, n, 16) for n in (5, 9)], [ref.unit_rows(rng, n, 16) for n in (8, 3)]
    qf, rf = _fine_inputs(3, (5, 9), 4, 16, "att"), _fine_inputs(4, (8, 3), 4, 16, "att")
    c = Ctx(qc, rc)
    try:
        pairs = [(0, 0), (1, 1)]
        c.set_fine(qf, rf, "att")
        assert c.fine_similarity(pairs, True)[0] == 0
        good_q = np.ascontiguousarray(np.concatenate(qf)[:, :, :8])
        good_r = np.ascontiguousarray(np.concatenate(rf)[:, :, :8])
        bad_q = good_q.copy()
        bad_q[3, 1, 2] = np.nan
        set_f16 = lambda q, r: c.L.vsc_tn_set_fine_f16(c.ctx, None if q is None else q.ctypes.data,
                                                       None if r is None else r.ctypes.data, 4, 8, 0, _lib.MEM_HOST)
        assert set_f16(bad_q, good_r) == _lib.VSC_ERR_INVALID and b"query" in c.L.vsc_last_error()
        assert c.L.vsc_tn_fine_bytes(c.ctx) == 0
        assert set_f16(good_q, None) == 0
        assert c.fine_similarity(pairs, True)[0] == _lib.VSC_ERR_INVALID and b"reference" in c.L.vsc_last_error()
        assert set_f16(None, good_r) == 0
        rc_, got, _ = c.fine_similarity(pairs, True)
        half = lambda v: ref.half_rounded(v[:, :, :8])
        assert rc_ == 0 and np.array_equal(helpers.bits(got[1]), helpers.bits(ref.fine_sim(half(qf[1]), half(rf[1]), "att", True)))
    finally:
        c.close()


# The converted-rows upload (bin: {0, 1} bytes -> +-1 fp32 -> packed rows) works in chunks of 64 MB of fp32, host and device
# sources alike: 262 144 rows at D = 64, which is 16 384 frames of 16 regions.  16 500 reference frames are the smallest
# side that needs a second chunk; video 1 lies across the boundary (frame 20 of its 40 is the chunk's first), video 3 is
# the last one, wholly inside the second chunk with the zero tail behind it.
MC_REGIONS, MC_DIM, MC_CHUNK_FRAMES = 16, 64, (64 << 20) // (64 * 4) // 16
MC_R_LENS = (MC_CHUNK_FRAMES - 20, 40, 60, 36)
MC_Q_LENS = (5, 9)
MC_PAIRS = [(0, 1), (1, 1), (0, 3), (1, 3)]


def test_stage1_upload_in_more_than_one_chunk(gpu, orc):
    import torch

    from vsc2022_amd import _lib

    assert sum(MC_R_LENS) == 16500 and sum(MC_R_LENS[:1]) < MC_CHUNK_FRAMES < sum(MC_R_LENS[:2])
    rng = np.random.default_rng(16384)
    qc, rc = [ref.unit_rows(rng, n, 8) for n in MC_Q_LENS], [ref.unit_rows(rng, n, 8) for n in MC_R_LENS]
    q_rows = rng.integers(0, 2, size=(sum(MC_Q_LENS), MC_REGIONS, MC_DIM), dtype=np.uint8)
    r_rows = rng.integers(0, 2, size=(sum(MC_R_LENS), MC_REGIONS, MC_DIM), dtype=np.uint8)
    qf, rf = np.split(q_rows, np.cumsum(MC_Q_LENS)[:-1]), np.split(r_rows, np.cumsum(MC_R_LENS)[:-1])
    want = {symmetric: [ref.fine_sim(qf[q], rf[r], "bin", symmetric) for q, r in MC_PAIRS] for symmetric in (False, True)}
    # include/vscmi.h: round_up(frames R + 64, 128) rows of round_up(fdim, 64) floats per side
    fine_bytes = sum((n * MC_REGIONS + 64 + 127) // 128 * 128 * 64 * 4 for n in (sum(MC_Q_LENS), sum(MC_R_LENS)))
    c = Ctx(qc, rc)
    try:
        for mem in ("host", "device"):
            if mem == "host":
                q_ptr, r_ptr, mem_id = q_rows.ctypes.data, r_rows.ctypes.data, _lib.MEM_HOST
            else:
                keep = torch.from_numpy(q_rows).to("cuda:0"), torch.from_numpy(r_rows).to("cuda:0")
                torch.cuda.synchronize()
                q_ptr, r_ptr, mem_id = keep[0].data_ptr(), keep[1].data_ptr(), _lib.MEM_DEVICE
            _lib.check(c.L.vsc_tn_set_fine(c.ctx, q_ptr, r_ptr, MC_REGIONS, MC_DIM, _lib.FINE_BIN, mem_id))
            assert c.L.vsc_tn_fine_bytes(c.ctx) == fine_bytes
            for symmetric in (False, True):
                rc_, got, _ = c.fine_similarity(MC_PAIRS, symmetric)
                assert rc_ == 0, c.L.vsc_last_error()
                for p, a, b in zip(MC_PAIRS, got, want[symmetric]):
                    assert np.array_equal(helpers.bits(a), helpers.bits(b)), (mem, p, symmetric, np.abs(a - b).max())
            # (the second upload must not pass on the first one's rows: both sides are overwritten in between)
            c.set_fine([np.zeros_like(v) for v in qf], [np.zeros_like(v) for v in rf], "bin")
            assert not np.array_equal(c.fine_similarity(MC_PAIRS[:1], True)[1][0], want[True][0])
    finally:
        c.close()


# ---- 2. stage 2 bits ------------------------------------------------------------------------------------------------

S2_Q_LENS = (40, 25, 64, 12, 300, 0, 70)
S2_R_LENS = (50, 31, 20, 45, 400, 90)
S2_PAIRS = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (0, 1), (2, 0), (5, 0), (1, 1), (3, 0), (6, 5), (6, 4)]


@pytest.fixture(scope="module")
def s2_inputs(orc):
    """Planted inputs (R = 4, D = 16) with a 300 x 400 pair for the HBM tile route, and F of every pair by the restatement."""
    qc, rc, qf, rf = ref.planted(17, S2_Q_LENS, S2_R_LENS, 64, 4, 16, "att")
    fine = {p: ref.fine_sim(qf[p[0]], rf[p[1]], "att", True) for p in set(S2_PAIRS)}
    return qc, rc, qf, rf, fine


@pytest.mark.parametrize("codec", ["Flat", "SQfp16"])
@pytest.mark.parametrize("params", [ref.REF_PARAMS, ref.SLAB_PARAMS], ids=["ref", "slab"])
def test_stage2_is_the_restatement(gpu, orc, s2_inputs, codec, params):
    qc, rc, qf, rf, fine = s2_inputs
    rc_seen = [ref.half_rounded(v) for v in rc] if codec == "SQfp16" else rc
    mats = [fine[p] for p in S2_PAIRS]
    c = Ctx(qc, rc, codec)
    try:
        n_found = 0
        for geometric_mean in (True, False):
            for bias in (0.0, 0.5):
                want = []
                for (q, r), f in zip(S2_PAIRS, mats):
                    s = ref.blend(f, orc.pair_sims(qc[q], rc_seen[r], bias)) if geometric_mean else f
                    want.append(ref.localise(s, params, bias))
                for device_slab in (False, True):
                    n_boxes, boxes, box_max = c.localize_fine(S2_PAIRS, mats, geometric_mean, params, bias, device_slab)
                    for k, (wb, ws) in enumerate(want):
                        assert boxes[k, :n_boxes[k]].tolist() == wb, (k, geometric_mean, bias, device_slab)
                        assert np.array_equal(helpers.bits(box_max[k, :n_boxes[k]]), helpers.bits(np.array(ws, dtype=F32)))
                n_found += sum(len(wb) for wb, _ in want)
        assert n_found >= 8
    finally:
        c.close()


@pytest.mark.parametrize("codec", ["Flat", "SQfp16"])
def test_stage2_from_the_hbm_state_slab(gpu, orc, s2_inputs, codec):
    """At top 16 / step 64 a pair of 59 query rows or more keeps its working state in HBM (tests/test_gpu_tn_params.py):
    the blend runs on that route's similarity slab as well; the 40- and 12-row pairs of the same call keep LDS state."""
    qc, rc, qf, rf, fine = s2_inputs
    rc_seen = [ref.half_rounded(v) for v in rc] if codec == "SQfp16" else rc
    params = dict(tn_top_k=16, tn_max_step=64, min_length=4)
    pairs = [(2, 2), (0, 0), (6, 5), (3, 3), (2, 0)]
    mats = [fine[p] for p in pairs]
    c = Ctx(qc, rc, codec)
    try:
        for geometric_mean in (True, False):
            n_boxes, boxes, box_max = c.localize_fine(pairs, mats, geometric_mean, params, 0.5, device_slab=True)
            for k, ((q, r), f) in enumerate(zip(pairs, mats)):
                s = ref.blend(f, orc.pair_sims(qc[q], rc_seen[r], 0.5)) if geometric_mean else f
                wb, ws = ref.localise(s, params, 0.5)
                assert boxes[k, :n_boxes[k]].tolist() == wb, (k, geometric_mean)
                assert np.array_equal(helpers.bits(box_max[k, :n_boxes[k]]), helpers.bits(np.array(ws, dtype=F32)))
    finally:
        c.close()


def test_stage2_feeds_match_rows(gpu, orc, s2_inputs):
    """Stage 1 in HBM -> stage 2 -> the rows of vsc_tn_match_rows, nothing but the box table on the host."""
    from vsc2022_amd import _lib

    qc, rc, qf, rf, fine = s2_inputs
    c = Ctx(qc, rc)
    try:
        c.set_fine(qf, rf, "att")
        rc_, got, _ = c.fine_similarity(S2_PAIRS, True, device_out=True)
        assert rc_ == 0
        for p, a in zip(S2_PAIRS, got):
            assert np.array_equal(helpers.bits(a), helpers.bits(fine[p])), p
        n_boxes, boxes, box_max = c.localize_fine(S2_PAIRS, got, True, ref.REF_PARAMS, 0.5, device_slab=True)
        q_ts = np.ascontiguousarray(np.stack([np.arange(sum(S2_Q_LENS)), np.arange(sum(S2_Q_LENS)) + 1.0], axis=1), dtype=np.float64)
        r_ts = np.ascontiguousarray(np.stack([np.arange(sum(S2_R_LENS)), np.arange(sum(S2_R_LENS)) + 1.0], axis=1), dtype=np.float64)
        _lib.check(c.L.vsc_tn_set_timestamps(c.ctx, q_ts.ctypes.data, r_ts.ctypes.data, _lib.MEM_HOST))
        cap = int(n_boxes.sum())
        assert cap >= 3
        pq, pr = (np.array(x, dtype=np.int32) for x in zip(*S2_PAIRS))
        pair, corners, score, times = (np.empty(cap, dtype=np.int32), np.empty((cap, 4), dtype=np.int32),
                                       np.empty(cap, dtype=F32), np.empty((cap, 4), dtype=np.float64))
        n_rows = ctypes.c_int64(0)
        _lib.check(c.L.vsc_tn_match_rows(c.ctx, pq.ctypes.data, pr.ctypes.data, len(S2_PAIRS), _lib.MEM_HOST, n_boxes.ctypes.data,
                                         boxes.ctypes.data, box_max.ctypes.data, _lib.MEM_HOST, pair.ctypes.data,
                                         corners.ctypes.data, score.ctypes.data, times.ctypes.data, cap, _lib.MEM_HOST,
                                         ctypes.byref(n_rows)))
        assert n_rows.value == cap
        want = [(k, boxes[k, b].tolist(), box_max[k, b]) for k in range(len(S2_PAIRS)) for b in range(n_boxes[k])]
        assert pair.tolist() == [w[0] for w in want] and corners.tolist() == [w[1] for w in want]
        assert np.array_equal(helpers.bits(score), helpers.bits(np.array([w[2] for w in want], dtype=F32)))
    finally:
        c.close()


# ---- 3. clip edges --------------------------------------------------------------------------------------------------

def test_clip_edges(gpu, orc):
    """F = 0 (bin complements), C < 1e-7 (negative coarse similarity at bias 0) and F, C equal to float32(1e-7) exactly."""
    tiny = F32(1e-7)
    rng = np.random.default_rng(21)
    qc = [ref.unit_rows(rng, 9, 64), ref.unit_rows(rng, 6, 64)]
    rc = [ref.unit_rows(rng, 11, 64), ref.unit_rows(rng, 7, 64)]
    rc[0][2] = -qc[0][4]  # C = -1 at bias 0
    rc[0][3] = 0.0        # C = bias exactly: with bias = float32(1e-7) the clip's own value
    qf = [rng.random((n, 4, 32)) > 0.5 for n in (9, 6)]
    rf = [rng.random((n, 4, 32)) > 0.5 for n in (11, 7)]
    qf[0][4] = qf[0][4, :1]
    rf[0][2] = ~qf[0][4]  # every region pair at -1: F0 = -1, F = 0
    c = Ctx(qc, rc)
    try:
        c.set_fine(qf, rf, "bin")
        pairs = [(0, 0), (1, 1), (0, 1)]
        rc_, fine, _ = c.fine_similarity(pairs, True)
        assert rc_ == 0 and fine[0][4, 2] == 0.0
        for (q, r), f in zip(pairs, fine):
            assert np.array_equal(helpers.bits(f), helpers.bits(ref.fine_sim(qf[q], rf[r], "bin", True)))
            f = f.copy()
            f[0, :] = tiny  # a row of F at the clip value exactly, one below and one above it
            f[0, 0], f[0, 1] = np.nextafter(tiny, F32(0)), np.nextafter(tiny, F32(1))
            for bias in (0.0, float(tiny), 0.5):
                coarse = orc.pair_sims(qc[q], rc[r], bias)
                if (q, r) == (0, 0):
                    assert coarse[4, 2] < 0 or bias == 0.5
                    assert coarse[0, 3] == F32(bias)
                got = c.similarity_fine(q, r, bias, f, True)
                assert np.array_equal(helpers.bits(got), helpers.bits(ref.blend(f, coarse))), (q, r, bias)
                assert np.array_equal(helpers.bits(c.similarity_fine(q, r, bias, f, False)), helpers.bits(f))
    finally:
        c.close()


# ---- 4. classes -----------------------------------------------------------------------------------------------------

def _class_case(kind, model, device, on_device, **kw):
    from vsc2022_amd.vsc.baseline.dns_baseline import VCSLLocalizationDnS
    from vsc2022_amd.vsc.metrics import CandidatePair

    qc, rc, qf, rf = ref.class_inputs(kind)
    (qv, qfv), (rv, rfv) = ref.video_features(qc, qf, "Q"), ref.video_features(rc, rf, "R")
    loc = VCSLLocalizationDnS(model, qfv, rfv, qv, rv, model_type="TN", tn_max_step=5, min_length=4, concurrency=16,
                              similarity_bias=0.5, device=device, on_device=on_device, **kw)
    cands = [CandidatePair(qv[q].video_id, rv[r].video_id, 1.0 - 0.01 * k) for k, (q, r) in enumerate(ref.CLASS_PAIRS)]
    return loc, cands, (qc, rc, qf, rf)


@pytest.mark.parametrize("kind", ["att", "bin"])
@pytest.mark.parametrize("geometric_mean", [True, False])
def test_class_with_a_torch_module_equals_the_host_route(gpu, kind, geometric_mean):
    import torch

    scripted = torch.jit.script(helpers.dns_standin(kind)).to("cuda")
    assert scripted.fg_type == kind
    host, cands, _ = _class_case(kind, scripted, "cuda", False, geometric_mean=geometric_mean)
    dev, _, _ = _class_case(kind, scripted, "cuda", True, geometric_mean=geometric_mean)
    want = host.localize_all(cands)
    got = dev.localize_all(cands)
    assert len(want) >= 5 and got == want
    assert dev.localize_table(cands).to_matches() == got
    assert [m for c in cands[:3] for m in dev.localize(c)] == dev.localize_all(cands[:3]) == host.localize_all(cands[:3])
    for c in cands[:3]:
        assert np.array_equal(helpers.bits(dev.similarity(c)), helpers.bits(host.similarity(c)))


@pytest.mark.parametrize("kind", ["att", "bin"])
def test_class_with_chamfer_is_the_restatement(gpu, orc, kind):
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity

    dev, cands, (qc, rc, qf, rf) = _class_case(kind, ChamferSimilarity(kind), "cpu", True)
    host, _, _ = _class_case(kind, ChamferSimilarity(kind), "cpu", False)
    assert dev.fine_bytes > 0
    got = dev.localize_all(cands)
    want = []
    for c, (q, r) in zip(cands, ref.CLASS_PAIRS):
        s = ref.blend(ref.fine_sim(qf[q], rf[r], kind, True), orc.pair_sims(qc[q], rc[r], 0.5))
        assert np.array_equal(helpers.bits(dev.similarity(c)), helpers.bits(s))
        boxes, scores = ref.localise(s, ref.REF_PARAMS, 0.5)
        want += [(c.query_id, c.ref_id, float(x1), float(x2 + 1), float(y1), float(y2 + 1), sc) for (x1, y1, x2, y2), sc in zip(boxes, scores)]
    assert len(want) >= 5
    assert [(m.query_id, m.ref_id, m.query_start, m.query_end, m.ref_start, m.ref_end) for m in got] == [w[:6] for w in want]
    assert np.array_equal(helpers.bits(np.array([m.score for m in got])), helpers.bits(np.array([w[6] for w in want])))
    assert dev.localize_table(cands).to_matches() == got
    by_host = host.localize_all(cands)
    assert [m._replace(score=0.0) for m in by_host] == [m._replace(score=0.0) for m in got]
    assert max(abs(float(a.score) - float(b.score)) for a, b in zip(by_host, got)) <= 4e-6


@pytest.mark.parametrize("tag", ["att", "bin", "att_plain"])
def test_class_with_chamfer_on_the_reference_goldens(gpu, tag):
    """tests/test_gpu_dns.py's fixtures and tolerances, through on_device=True."""
    from vsc2022_amd import synth
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity, VCSLLocalizationDnS
    from vsc2022_amd.vsc.index import VideoFeature
    from vsc2022_amd.vsc.metrics import CandidatePair

    fx = helpers.load("g9_dns_" + tag)
    fg_type = str(fx["fg_type"])
    q, r, qfine, rfine = helpers.g9_inputs(fg_type)
    qc, rc = synth.to_video_features(q, VideoFeature), synth.to_video_features(r, VideoFeature)
    qf = {v.video_id: VideoFeature(video_id=v.video_id, timestamps=v.timestamps, feature=f) for v, f in zip(qc, qfine)}
    rf = {v.video_id: VideoFeature(video_id=v.video_id, timestamps=v.timestamps, feature=f) for v, f in zip(rc, rfine)}
    loc = VCSLLocalizationDnS(ChamferSimilarity(fg_type), qf, rf, qc, rc, model_type="TN", tn_max_step=5, min_length=4,
                              concurrency=16, similarity_bias=0.5, device="cpu", symmetric=bool(fx["symmetric"]),
                              geometric_mean=bool(fx["geometric_mean"]), on_device=True)
    cands = [CandidatePair(str(a), str(b), float(s)) for a, b, s in zip(fx["cand_q"], fx["cand_r"], fx["cand_s"])]
    cuts = np.r_[0, np.cumsum(fx["sim_shapes"].prod(axis=1))]
    for k in range(0, len(cands), 5):
        want = fx["sims"][cuts[k]:cuts[k + 1]].reshape(fx["sim_shapes"][k])
        got = loc.similarity(cands[k])
        assert got.shape == want.shape and np.abs(got - want).max() < 2e-6, (k, np.abs(got - want).max())
    matches = loc.localize_all(cands)
    rows = fx["m_rows"]
    assert len(matches) == len(rows)
    assert [str(m.query_id) for m in matches] == list(fx["m_q"]) and [str(m.ref_id) for m in matches] == list(fx["m_r"])
    got = np.array([[m.score, m.query_start, m.query_end, m.ref_start, m.ref_end] for m in matches], dtype=np.float64)
    assert np.array_equal(got[:, 1:], rows[:, 1:])
    assert np.abs(got[:, 0] - rows[:, 0]).max() < 4e-6


# ---- 5. handle reuse ------------------------------------------------------------------------------------------------

def _reuse_sequence():
    """Two batches of different sizes on one context, a new query side (the fine call is refused until its fine descriptors
    are set again), and the results of a fresh context afterwards."""
    from vsc2022_amd import _lib

    qc, rc, qf, rf = ref.planted(33, (40, 25, 64, 12), (50, 31, 20), 64, 9, 20, "att")
    qc2, _, qf2, _ = ref.planted(34, (18, 70), (50, 31, 20), 64, 9, 20, "att")
    big = [(0, 0), (1, 1), (2, 2), (3, 0), (2, 1), (0, 2), (1, 0)]
    small = [(3, 2), (0, 0)]
    later = [(0, 0), (1, 1), (1, 2)]

    def run(c, pairs, q_fine, q_coarse):
        rc_, fine, _ = c.fine_similarity(pairs, True, device_out=True)
        assert rc_ == 0, c.L.vsc_last_error()
        for (q, r), f in zip(pairs, fine):
            assert np.array_equal(helpers.bits(f), helpers.bits(ref.fine_sim(q_fine[q], rf[r], "att", True))), (q, r)
        n_boxes, boxes, box_max = c.localize_fine(pairs, fine, True, ref.REF_PARAMS, 0.5, device_slab=True)
        n = 0
        for k, ((q, r), f) in enumerate(zip(pairs, fine)):
            wb, ws = ref.localise(ref.blend(f, orc.pair_sims(q_coarse[q], rc[r], 0.5)), ref.REF_PARAMS, 0.5)
            assert boxes[k, :n_boxes[k]].tolist() == wb
            assert np.array_equal(helpers.bits(box_max[k, :n_boxes[k]]), helpers.bits(np.array(ws, dtype=F32)))
            n += len(wb)
        return n_boxes, boxes, box_max, n

    import oracle as orc

    orc.build()
    c = Ctx(qc, rc)
    try:
        c.set_fine(qf, rf, "att")
        assert run(c, big, qf, qc)[3] >= 2
        run(c, small, qf, qc)
        run(c, big, qf, qc)
        c.set_queries(qc2)
        assert c.fine_similarity(later, True)[0] == _lib.VSC_ERR_INVALID
        c.set_fine(qf2, None, "att")
        reused = run(c, later, qf2, qc2)
    finally:
        c.close()
    fresh_ctx = Ctx(qc2, rc)
    try:
        fresh_ctx.set_fine(qf2, rf, "att")
        fresh = run(fresh_ctx, later, qf2, qc2)
    finally:
        fresh_ctx.close()
    assert np.array_equal(reused[0], fresh[0])  # (the slots past a pair's box count are not written)
    for k, n in enumerate(fresh[0]):
        assert np.array_equal(reused[1][k, :n], fresh[1][k, :n])
        assert np.array_equal(helpers.bits(reused[2][k, :n]), helpers.bits(fresh[2][k, :n]))


def test_handle_reuse(gpu, orc):
    _reuse_sequence()


def test_handle_reuse_with_poisoned_allocations(gpu):
    """The same sequence under VSC_POISON_ALLOC=1 in a fresh process: every new device buffer starts as 0xFF bytes."""
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_dns_device as t; t._reuse_sequence(); print('reuse ok')" % (
        ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, VSC_POISON_ALLOC="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "reuse ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
