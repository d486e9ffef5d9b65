"""GPU: the per-batch plumbing of the Temporal-Network contexts (csrc/api_tn.hip) -- pair lists and box tables in host or
device memory, the forward-sim forms of both runners, and the device buffers the entry points of one context share.

One Flat and one SQfp16 context over six query and six reference videos (dim 20, padded to 64); one pair list that holds
every launch bucket of tn_run_buckets and align_run_buckets at once (restated and asserted below, from the constants in
csrc/api_tn.hip, csrc/kernels.h and tests/tn_cases.py).  Every comparison is exact.  A box table is compared in its
defined part: all of `nbox` and `status`, and the first `nbox[p]` slots of `boxes` / `boxmax` -- the kernels write no
other slot, and a host caller gets the staging buffer's earlier contents there."""
import ctypes
import functools

import numpy as np
import pytest

from codec_rows import dec, unit
from helpers import bits
from tn_cases import state_bytes


DIM = 20
Q_LENS = (0, 3, 40, 64, 200, 300)
R_LENS = (0, 5, 64, 100, 700, 33000)
# (query, reference) ordinals            frames      tn_run_buckets        align_run_buckets (fused)
PAIRS = ((2, 2),                       # 40 x 64     0 (LDS tile <= 4096)  DP 1, DTW 0
         (4, 3),                       # 200 x 100   1 (LDS tile <= 24576) status 1 alone: more than ALIGN_MAX_CELLS cells
         (2, 4),                       # 40 x 700    2 (slab)              status 1 alone
         (1, 5),                       # 3 x 33000   3 (HBM state: lr > 32767)  status 1 alone
         (1, 1),                       # 3 x 5       0                     DP 0, DTW 0
         (3, 3),                       # 64 x 100    1                     DP 2, DTW 1
         (5, 1),                       # 300 x 5     2 (lq > 256)          DP 0, DTW 0
         (0, 2),                       # 0 x 64      0                     status 0 alone: an empty query
         (2, 0))                       # 40 x 0      0                     status 0 alone: an empty reference
TN_KW = dict(min_length=1)             # (tn_top_k 5, tn_max_step 10: the defaults the bucket limits are quoted for)
ALIGN_KW = dict(discontinue=3, min_sim=0.5, min_length=3, max_iou=0.3)


def tn_bucket(lq, lr, top=5, ms=10, fused=True):
    """tn_run_buckets' choice (csrc/api_tn.hip), restated."""
    tile_ok = [state_bytes(m, top, ms) + 4 * t <= 158 * 1024 for m, t in ((64, 4096), (256, 24576))]
    if lq * top + 1 > 32767 or lr > 32767 or state_bytes(max(lq, 1), top, ms) > 150 * 1024:
        return 3
    if lq <= 64 and (not fused or (tile_ok[0] and lq * lr <= 4096)):
        return 0
    if lq <= 256 and (not fused or (tile_ok[1] and lq * lr <= 24576)):
        return 1
    return 2


def align_class(dtw, lq, lr, fused=True):
    """The LDS class align_run_buckets puts a pair in: align_layout(...).total (csrc/kernels.h) against 24 / 64 / 150 KiB;
    None for a pair the kernel answers by its status alone."""
    from vsc2022_amd import _lib

    cells, edge = lq * lr, lq + lr
    if lq == 0 or lr == 0 or cells > _lib.ALIGN_MAX_CELLS:
        return None
    b = (3 * (min(lq, lr) + 1) * 8 + (edge // 2 + 1) * 16) if dtw else (cells * 8 + 256)
    b += (cells * 4 if fused else 0) + 256 + (cells + edge if dtw else cells * 2 + edge)
    b = (b + 15) & ~15
    assert b <= 150 * 1024
    return 0 if b <= 24 * 1024 else (1 if b <= 64 * 1024 else 2)


def test_the_pair_list_holds_every_bucket():
    shapes = [(Q_LENS[q], R_LENS[r]) for q, r in PAIRS]
    assert [tn_bucket(*s) for s in shapes] == [0, 1, 2, 3, 0, 1, 2, 0, 0]
    assert [align_class(False, *s) for s in shapes] == [1, None, None, None, 0, 2, 0, None, None]
    # (DTW keeps 5 B per cell + 9 B per edge frame: with these videos no pair of at most ALIGN_MAX_CELLS cells passes 64 KiB)
    assert [align_class(True, *s) for s in shapes] == [0, None, None, None, 0, 1, 0, None, None]


@functools.lru_cache(maxsize=None)
def videos():
    """(query videos, reference videos): unit rows, with a noised copy planted in every pair of PAIRS that has frames."""
    rng = np.random.default_rng(417)
    q = [unit(rng, n, DIM) for n in Q_LENS]
    r = [unit(rng, n, DIM) for n in R_LENS]

    def plant(dst, d0, src, s0, n):
        x = src[s0:s0 + n] + np.float32(0.05) * rng.standard_normal((n, DIM)).astype(np.float32)
        dst[d0:d0 + n] = x / np.linalg.norm(x, axis=1, keepdims=True)

    plant(q[2], 5, r[2], 20, 30)        # 40 x 64
    plant(r[4], 300, q[2], 0, 40)       # 40 x 700
    plant(q[4], 60, r[3], 10, 80)       # 200 x 100
    plant(q[3], 2, r[3], 30, 60)        # 64 x 100
    plant(r[5], 20000, q[1], 0, 3)      # 3 x 33000
    plant(r[1], 0, q[5], 100, 5)        # 300 x 5 (and 3 x 5: noise)
    for v in q + r:
        v.setflags(write=False)
    return q, r


def _offsets(vs):
    return np.r_[0, np.cumsum([len(v) for v in vs])].astype(np.int64)


def _held(a, device):
    """(what keeps the memory alive, address, VSC_MEM_*) of a numpy array as it is, or copied to the GPU."""
    from vsc2022_amd import _lib

    if not device:
        return a, a.ctypes.data, _lib.MEM_HOST
    import torch

    t = torch.from_numpy(a).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr(), _lib.MEM_DEVICE


def _back(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _table(nbox, boxes, bmax, status=None):
    """The defined part of a box table, as arrays that compare with np.array_equal."""
    nbox = _back(nbox)
    valid = np.arange(16)[None, :] < nbox[:, None]
    out = {"nbox": nbox, "boxes": _back(boxes)[valid], "boxmax": bits(_back(bmax)[valid])}
    if status is not None:
        out["status"] = _back(status)
    return out


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


class Ctx:
    def __init__(self, codec):
        from vsc2022_amd import _lib
        from vsc2022_amd.vcsl.vta import tn_params

        self._lib, self.L = _lib, _lib.lib()
        q, r = videos()
        self.q_off, self.r_off = _offsets(q), _offsets(r)
        q_rows, r_rows = np.concatenate(q), np.concatenate(r)
        self.ctx = ctypes.c_void_p()
        _lib.check(self.L.vsc_tn_create_codec(q_rows.ctypes.data, self.q_off.ctypes.data, len(q), r_rows.ctypes.data, 0,
                                              self.r_off.ctypes.data, len(r), DIM, _lib.MEM_HOST, _lib.MEM_HOST, _lib.codec_id(codec), 0,
                                              ctypes.byref(self.ctx)))
        self.pq, self.pr = (np.array(x, dtype=np.int32) for x in zip(*PAIRS))
        self.n = len(PAIRS)
        self.tn_prm = tn_params(**TN_KW)

    def close(self):
        self.L.vsc_tn_destroy(self.ctx)

    def _outputs(self, device, status):
        """Canary-filled outputs: [(holder, address)] of nbox, boxes, boxmax (, status) and their memory kind."""
        arrays = [np.full(self.n, -7, np.int32), np.full((self.n, 16, 4), -7, np.int32), np.full((self.n, 16), -7.25, np.float32)]
        if status:
            arrays.append(np.full(self.n, -7, np.int32))
        held = [_held(a, device) for a in arrays]
        return [h[0] for h in held], [h[1] for h in held], held[0][2]

    def localize(self, pairs_dev=False, out_dev=False):
        pq, pr = _held(self.pq, pairs_dev), _held(self.pr, pairs_dev)
        out, addr, mem = self._outputs(out_dev, False)
        self._lib.check(self.L.vsc_tn_localize(self.ctx, pq[1], pr[1], self.n, pq[2], ctypes.byref(self.tn_prm), 0.0, *addr, mem))
        return _table(*out)

    def align(self, method, pairs_dev=False, out_dev=False):
        pq, pr = _held(self.pq, pairs_dev), _held(self.pr, pairs_dev)
        out, addr, mem = self._outputs(out_dev, True)
        self._lib.check(self.L.vsc_tn_align(self.ctx, pq[1], pr[1], self.n, pq[2], ctypes.byref(align_params(method)), 0.0, *addr, mem))
        return _table(*out)

    def similarity(self, p):
        q, r = PAIRS[p]
        out = np.zeros((Q_LENS[q], R_LENS[r]), np.float32)
        self._lib.check(self.L.vsc_tn_similarity(self.ctx, q, r, 0.0, out.ctypes.data, out.size, None, None))
        return out


def align_params(method):
    from vsc2022_amd import _lib

    return _lib.AlignParams(method, ALIGN_KW["discontinue"], ALIGN_KW["min_length"], 10 if method == _lib.ALIGN_DP else 0,
                            ALIGN_KW["min_sim"], ALIGN_KW["max_iou"])


@pytest.fixture(scope="module", params=["Flat", "SQfp16"])
def ctx(gpu, request):
    c = Ctx(request.param)
    c.codec = request.param
    yield c
    c.close()


@pytest.fixture(scope="module")
def sims(ctx):
    """vsc_tn_similarity's matrix of every pair of PAIRS (module-wide per context, never modified)."""
    mats = [ctx.similarity(p) for p in range(len(PAIRS))]
    for m in mats:
        m.setflags(write=False)
    return mats


def _tn_oracle(orc, codec):
    q, r = videos()
    want_n, want_boxes, want_max = [], [], []
    for qv, rv in PAIRS:
        if Q_LENS[qv] == 0 or R_LENS[rv] == 0:
            want_n.append(0)
            continue
        s = orc.pair_sims(q[qv], r[rv] if codec == "Flat" else dec(r[rv]), 0.0)
        boxes = orc.tn(s, **TN_KW)
        want_n.append(len(boxes))
        want_boxes += boxes
        want_max += [s[x1:x2, y1:y2].max() for x1, y1, x2, y2 in boxes]   # (MaxSim's half-open slice: helpers.py)
    return {"nbox": np.array(want_n, np.int32), "boxes": np.array(want_boxes, np.int32).reshape(-1, 4),
            "boxmax": bits(np.array(want_max, np.float32))}


@pytest.mark.gpu
def test_localize_in_every_memory_kind_is_the_oracle(ctx, orc):
    first = ctx.localize()
    _same(first, _tn_oracle(orc, ctx.codec), "host / host against the oracle")
    assert first["nbox"][:7].all() and not first["nbox"][7:].any(), first["nbox"]   # a box from every bucket: nothing vacuous
    for pairs_dev, out_dev in ((False, True), (True, False), (True, True)):
        _same(ctx.localize(pairs_dev, out_dev), first, (pairs_dev, out_dev))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["DTW", "DP"])
def test_align_in_every_memory_kind_is_the_host_function(ctx, sims, name):
    from vsc2022_amd import _lib
    from vsc2022_amd.vcsl import aligners

    method = {"DTW": _lib.ALIGN_DTW, "DP": _lib.ALIGN_DP}[name]
    kw = dict(ALIGN_KW, max_path=10) if name == "DP" else ALIGN_KW
    first = ctx.align(method)
    want_n, want_boxes, want_status = [], [], []
    for (qv, rv), s in zip(PAIRS, sims):
        host = [] if s.size == 0 or s.size > _lib.ALIGN_MAX_CELLS else getattr(aligners, name.lower())(s, **kw)
        want_status.append(1 if s.size > _lib.ALIGN_MAX_CELLS else (2 if len(host) > _lib.TN_MAX_BOXES else 0))
        if want_status[-1] == 0:
            want_boxes += host
        want_n.append(len(host) if want_status[-1] == 0 else 0)
    assert want_status == [0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert np.array_equal(first["status"], want_status) and np.array_equal(first["nbox"], want_n), (first["status"], first["nbox"], want_n)
    assert np.array_equal(first["boxes"], np.array(want_boxes, np.int32).reshape(-1, 4))
    # the planted copies are found in every LDS class that has a pair (40 x 64, 64 x 100; DP also the five frames of 300 x 5,
    # which DTW's one warping path over the whole matrix does not isolate)
    assert first["nbox"][0] and first["nbox"][5] and (name == "DTW" or first["nbox"][6]), first["nbox"]
    for pairs_dev, out_dev in ((False, True), (True, False), (True, True)):
        _same(ctx.align(method, pairs_dev, out_dev), first, (name, pairs_dev, out_dev))


@pytest.mark.gpu
def test_forward_sim_forms_equal_the_fused_ones(ctx, sims):
    from vsc2022_amd import _lib
    from vsc2022_amd.vcsl.vta import pack_sims

    _, flat, off, lq, lr, nbox, boxes, bmax = pack_sims(sims)
    n = len(sims)
    _lib.check(ctx.L.vsc_tn_forward_sim(flat.ctypes.data, off.ctypes.data, lq.ctypes.data, lr.ctypes.data, n, ctypes.byref(ctx.tn_prm),
                                        nbox.ctypes.data, boxes.ctypes.data, bmax.ctypes.data, 0))
    _same(_table(nbox, boxes, bmax), ctx.localize(), "vsc_tn_forward_sim")
    for method in (_lib.ALIGN_DTW, _lib.ALIGN_DP):
        status = np.full(n, -7, np.int32)
        _lib.check(ctx.L.vsc_align_forward_sim(flat.ctypes.data, off.ctypes.data, lq.ctypes.data, lr.ctypes.data, n,
                                               ctypes.byref(align_params(method)), nbox.ctypes.data, boxes.ctypes.data, bmax.ctypes.data,
                                               status.ctypes.data, 0))
        _same(_table(nbox, boxes, bmax, status), ctx.align(method), ("vsc_align_forward_sim", method))


@pytest.mark.gpu
def test_entry_points_of_one_context_share_their_buffers(ctx):
    """localize -> align -> set_timestamps -> match_rows -> set_fine -> fine_similarity -> localize_fine -> localize on ONE
    context: the pair lists (d_pq, d_pr), the box table (d_nbox, d_boxes, d_bmax), the work list and the slab are the same
    buffers throughout, and the last localisation is the first."""
    _lib, L, n = ctx._lib, ctx.L, ctx.n
    first = ctx.localize()
    ctx.align(_lib.ALIGN_DP)
    q_ts, r_ts = (np.stack([np.arange(o[-1], dtype=np.float64), np.arange(1, o[-1] + 1, dtype=np.float64)], axis=1)
                  for o in (ctx.q_off, ctx.r_off))
    _lib.check(L.vsc_tn_set_timestamps(ctx.ctx, q_ts.ctypes.data, r_ts.ctypes.data, _lib.MEM_HOST))
    # match rows of the first localisation's table (slots beyond nbox zeroed: the input is what a caller would hold)
    nbox = first["nbox"]
    valid = np.arange(16)[None, :] < nbox[:, None]
    boxes, bmax = np.zeros((n, 16, 4), np.int32), np.zeros((n, 16), np.float32)
    boxes[valid], bmax[valid] = first["boxes"], first["boxmax"].view(np.float32)
    total = int(nbox.sum())
    rows = []
    for device in (False, True):
        cols = [_held(a, device) for a in (np.full(total, -7, np.int32), np.full((total, 4), -7, np.int32),
                                           np.full(total, -7.25, np.float32), np.full((total, 4), -7.25, np.float64))]
        n_rows = ctypes.c_int64(-1)
        _lib.check(L.vsc_tn_match_rows(ctx.ctx, ctx.pq.ctypes.data, ctx.pr.ctypes.data, n, _lib.MEM_HOST, nbox.ctypes.data,
                                       boxes.ctypes.data, bmax.ctypes.data, _lib.MEM_HOST, *(c[1] for c in cols), total, cols[0][2],
                                       ctypes.byref(n_rows)))
        assert n_rows.value == total
        rows.append([_back(c[0]) for c in cols])
    for host, dev in zip(*rows):
        assert host.tobytes() == dev.tobytes()
    assert np.array_equal(rows[0][0], np.repeat(np.arange(n, dtype=np.int32), nbox)) and np.array_equal(rows[0][1], first["boxes"])
    # fine descriptors: att, 4 regions of fdim 20 per frame
    rng = np.random.default_rng(418)
    qf, rf = (unit(rng, int(o[-1]) * 4, DIM) for o in (ctx.q_off, ctx.r_off))
    _lib.check(L.vsc_tn_set_fine(ctx.ctx, qf.ctypes.data, rf.ctypes.data, 4, DIM, _lib.FINE_ATT, _lib.MEM_HOST))
    cells = np.array([Q_LENS[q] * R_LENS[r] for q, r in PAIRS], dtype=np.int64)
    off = np.r_[0, np.cumsum(cells)].astype(np.int64)
    fine = np.full(int(off[-1]) + 1, -7.25, np.float32)
    _lib.check(L.vsc_tn_fine_similarity(ctx.ctx, ctx.pq.ctypes.data, ctx.pr.ctypes.data, n, _lib.MEM_HOST, 0, fine.ctypes.data,
                                        off.ctypes.data, int(off[-1]), _lib.MEM_HOST))
    assert fine[-1] == np.float32(-7.25) and (np.abs(fine[:-1]) <= 1.0 + 1e-5).all()   # every cell written: unit rows
    got = {}
    for geometric in (1, 0):
        out = [np.full(n, -7, np.int32), np.full((n, 16, 4), -7, np.int32), np.full((n, 16), -7.25, np.float32)]
        _lib.check(L.vsc_tn_localize_fine(ctx.ctx, ctx.pq.ctypes.data, ctx.pr.ctypes.data, n, _lib.MEM_HOST, fine.ctypes.data,
                                          off.ctypes.data, _lib.MEM_HOST, geometric, ctypes.byref(ctx.tn_prm), 0.0,
                                          *(a.ctypes.data for a in out), _lib.MEM_HOST))
        got[geometric] = _table(*out)
    # the plain form aligns the fine matrices as they are: vsc_tn_forward_sim on them
    lq, lr = (np.array([lens[v] for v in col], np.int32) for lens, col in ((Q_LENS, ctx.pq), (R_LENS, ctx.pr)))
    out = [np.full(n, -7, np.int32), np.full((n, 16, 4), -7, np.int32), np.full((n, 16), -7.25, np.float32)]
    _lib.check(L.vsc_tn_forward_sim(fine.ctypes.data, off.ctypes.data, lq.ctypes.data, lr.ctypes.data, n, ctypes.byref(ctx.tn_prm),
                                    *(a.ctypes.data for a in out), 0))
    _same(got[0], _table(*out), "vsc_tn_localize_fine, plain")
    assert ((got[1]["nbox"] >= 0) & (got[1]["nbox"] <= 16)).all()
    _same(ctx.localize(), first, "the localisation after every other entry point")
