"""GPU: the match-rows stage (csrc/match_rows.hip behind vsc_tn_set_timestamps / vsc_tn_match_rows) and everything built on
it -- `VCSLLocalization.localize_table`, `sscd_baseline.localize_table`, `DeviceMatcher.match(rows=True)` / `match_table`.

The contract is exact (copies and gathers): every comparison below is bit for bit.  The kernels are checked against the numpy
restatement of tests/match_rows_ref.py (itself pinned against the per-box loop in tests/test_match_table_host.py); the Python
layers against `localize_all` / `localize_and_verify`, row for row and byte for byte."""
import ctypes
import functools
import io
import itertools

import numpy as np
import pytest

import match_rows_ref as mr
from helpers import g8_inputs, load, videos

pytestmark = pytest.mark.gpu

# edges of a wave (63 / 64 / 65), of a workgroup = the scan's tile of 256 pairs (255 / 256 / 257), of the carry pass's chunk
# of 256 tiles (65 535 / 65 536 / 65 537: the second level of carry), one size well beyond it
N_PAIRS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537, 200003]
CANARY_I, CANARY_F = -1234567, -7.25


class _Ctx:
    """A Temporal-Network context over the videos of match_rows_ref.video_tables (descriptors: zeros, never looked at)."""

    def __init__(self, timestamps=True):
        from vsc2022_amd import _lib

        self.q_off, self.r_off, self.q_ts, self.r_ts = mr.video_tables()
        self.h = ctypes.c_void_p()
        qf, rf = np.zeros((int(self.q_off[-1]), 4), np.float32), np.zeros((int(self.r_off[-1]), 4), np.float32)
        _lib.check(_lib.lib().vsc_tn_create(qf.ctypes.data, self.q_off.ctypes.data, len(self.q_off) - 1, rf.ctypes.data,
                                            self.r_off.ctypes.data, len(self.r_off) - 1, 4, _lib.MEM_HOST, 0, ctypes.byref(self.h)))
        if timestamps:
            _lib.check(_lib.lib().vsc_tn_set_timestamps(self.h, self.q_ts.ctypes.data, self.r_ts.ctypes.data, _lib.MEM_HOST))

    def close(self):
        from vsc2022_amd import _lib

        _lib.lib().vsc_tn_destroy(self.h)


@pytest.fixture(scope="module", autouse=True)
def _hand_back_cached_blocks():
    """The device cases leave canaries and out-of-range corners behind in the blocks torch's caching allocator keeps when
    their tensors die.  Hand the blocks back when the module ends: a later test's `torch.empty` must not find them (the
    slots of a box table beyond `nbox` are whatever the buffer held)."""
    yield
    import gc

    import torch

    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def ctx(gpu):
    c = _Ctx()
    yield c
    c.close()


def _run(c, table, cap, device, count_only=False, slack=3):
    """One vsc_tn_match_rows call with everything in host memory or everything in HBM; outputs pre-filled with canaries.
    Returns (rc, n_rows, (pair, box, score, times) as numpy arrays of cap + slack rows)."""
    import torch

    from vsc2022_amd import _lib

    n = len(table[0])
    rows = max(cap, 0) + slack
    outs = [np.full(rows, CANARY_I, np.int32), np.full((rows, 4), CANARY_I, np.int32), np.full(rows, CANARY_F, np.float32),
            np.full((rows, 4), CANARY_F, np.float64)]
    if device:
        dev = torch.device("cuda", 0)
        ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in table]
        outs_d = [torch.from_numpy(a).to(dev) for a in outs]
        torch.cuda.synchronize()
        in_ptr, out_ptr, mem = [t.data_ptr() if t.numel() else None for t in ins], [t.data_ptr() for t in outs_d], _lib.MEM_DEVICE
    else:
        ins = [np.ascontiguousarray(a) for a in table]
        in_ptr, out_ptr, mem = [a.ctypes.data for a in ins], [a.ctypes.data for a in outs], _lib.MEM_HOST
    if count_only:
        out_ptr, cap = [None] * 4, 0
    n_rows = ctypes.c_int64(-1)
    rc = _lib.lib().vsc_tn_match_rows(c.h, in_ptr[0], in_ptr[1], n, mem, in_ptr[2], in_ptr[3], in_ptr[4], mem, out_ptr[0], out_ptr[1],
                                      out_ptr[2], out_ptr[3], cap, mem, ctypes.byref(n_rows))
    if device:
        outs = [t.cpu().numpy() for t in outs_d]
    return rc, n_rows.value, outs


def _canary(outs, first):
    return all((a[first:] == (CANARY_I if a.dtype == np.int32 else CANARY_F)).all() for a in outs)


@pytest.mark.parametrize("pattern", mr.PATTERNS)
@pytest.mark.parametrize("n_pairs", N_PAIRS)
def test_kernel_is_the_numpy_restatement(ctx, n_pairs, pattern):
    from vsc2022_amd import _lib

    table = mr.box_table(n_pairs, pattern, ctx.q_off, ctx.r_off)
    want = mr.rows(*table, ctx.q_off, ctx.r_off, ctx.q_ts, ctx.r_ts)
    need = len(want[0])
    assert need == int(table[2].sum())
    if pattern == "full":
        assert need == 16 * n_pairs
    if pattern == "uniform" and n_pairs > 64:
        assert 0 < need < 16 * n_pairs and (want[1][:, 0] == 0).any()
    for device in (False, True):
        rc, n_rows, outs = _run(ctx, table, need, device)
        assert rc == _lib.VSC_OK, (device, _lib.lib().vsc_last_error())
        assert n_rows == need
        assert np.array_equal(outs[0][:need], want[0]) and np.array_equal(outs[1][:need], want[1]), device
        assert np.array_equal(outs[2][:need].view(np.uint32), want[2].view(np.uint32)), device
        assert np.array_equal(outs[3][:need].view(np.uint64), want[3].view(np.uint64)), device
        assert _canary(outs, need), device  # the slack rows behind the table
        rc, n_rows, _ = _run(ctx, table, 0, device, count_only=True)
        assert (rc, n_rows) == (_lib.VSC_OK, need), device
        if need:
            rc, n_rows, outs = _run(ctx, table, need - 1, device)
            assert rc == _lib.VSC_ERR_CAPACITY and n_rows == need, device
            assert _canary(outs, 0), device  # nothing written anywhere


def test_out_box_may_be_null_and_the_launches_are_accounted(ctx):
    from vsc2022_amd import _lib

    L = _lib.lib()
    table = mr.box_table(300, "uniform", ctx.q_off, ctx.r_off)
    want = mr.rows(*table, ctx.q_off, ctx.r_off, ctx.q_ts, ctx.r_ts)
    need = len(want[0])
    pair, score, times = np.empty(need, np.int32), np.empty(need, np.float32), np.empty((need, 4), np.float64)
    n_rows = ctypes.c_int64(0)
    ms, calls, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    _lib.check(L.vsc_aux_profile(1))
    try:
        _lib.check(L.vsc_aux_profile_read(3, None, None, None, 1))
        _lib.check(L.vsc_tn_match_rows(ctx.h, *(a.ctypes.data for a in table[:2]), 300, _lib.MEM_HOST, *(a.ctypes.data for a in table[2:]),
                                       _lib.MEM_HOST, pair.ctypes.data, None, score.ctypes.data, times.ctypes.data, need, _lib.MEM_HOST,
                                       ctypes.byref(n_rows)))
        _lib.check(L.vsc_aux_profile_read(3, ctypes.byref(ms), ctypes.byref(calls), ctypes.byref(by), 1))
    finally:
        _lib.check(L.vsc_aux_profile(0))
    assert n_rows.value == need and np.array_equal(pair, want[0]) and np.array_equal(times, want[3])
    assert calls.value == 2 and ms.value > 0.0 and by.value > 332.0 * 300  # the scan and the row pass


BAD = {
    "nbox 17": lambda t, c: t[2].__setitem__(4, 17),
    "nbox -1": lambda t, c: t[2].__setitem__(4, -1),
    "corner == L (query)": lambda t, c: t[3].__setitem__((4, 0, 2), int(np.diff(c.q_off)[t[0][4]])),
    "corner == L (ref)": lambda t, c: t[3].__setitem__((4, 1, 1), int(np.diff(c.r_off)[t[1][4]])),
    "negative corner": lambda t, c: t[3].__setitem__((4, 0, 0), -1),
    "query ordinal == n": lambda t, c: t[0].__setitem__(4, len(c.q_off) - 1),
    "ref ordinal == n": lambda t, c: t[1].__setitem__(4, len(c.r_off) - 1),
    "negative ordinal": lambda t, c: t[0].__setitem__(4, -2),
}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("bad", sorted(BAD))
def test_out_of_range_inputs_are_refused_not_read(ctx, bad, device):
    """Host memory: checked before anything is launched.  Device memory: the kernels skip the row and raise the error
    word.  Either way VSC_ERR_INVALID, and the rows of the untouched pairs of a following call are still right."""
    from vsc2022_amd import _lib

    table = [a.copy() for a in mr.box_table(40, "full", ctx.q_off, ctx.r_off)]
    BAD[bad](table, ctx)
    rc, _, outs = _run(ctx, table, 16 * 40, device)
    assert rc == _lib.VSC_ERR_INVALID, bad
    with pytest.raises(ValueError):
        _lib.check(rc)
    if not device:
        assert _canary(outs, 0)  # refused before a launch
    good = mr.box_table(40, "full", ctx.q_off, ctx.r_off)
    rc, n_rows, outs = _run(ctx, good, 16 * 40, device)
    assert (rc, n_rows) == (_lib.VSC_OK, 16 * 40)
    assert np.array_equal(outs[3][:n_rows], mr.rows(*good, ctx.q_off, ctx.r_off, ctx.q_ts, ctx.r_ts)[3])


def test_a_missing_timestamp_table_is_refused(gpu):
    from vsc2022_amd import _lib

    c = _Ctx(timestamps=False)
    try:
        table = mr.box_table(10, "full", c.q_off, c.r_off)
        L = _lib.lib()
        assert _run(c, table, 160, False)[0] == _lib.VSC_ERR_INVALID
        assert "query timestamp table" in L.vsc_last_error().decode()
        assert _run(c, table, 0, False, count_only=True)[:2] == (_lib.VSC_OK, 160)  # the count needs no table
        _lib.check(L.vsc_tn_set_timestamps(c.h, c.q_ts.ctypes.data, None, _lib.MEM_HOST))
        assert _run(c, table, 160, True)[0] == _lib.VSC_ERR_INVALID
        assert "reference timestamp table" in L.vsc_last_error().decode()
        _lib.check(L.vsc_tn_set_timestamps(c.h, None, c.r_ts.ctypes.data, _lib.MEM_HOST))  # (the query side is left as it is)
        rc, n_rows, outs = _run(c, table, 160, True)
        assert (rc, n_rows) == (_lib.VSC_OK, 160)
        assert np.array_equal(outs[3][:160], mr.rows(*table, c.q_off, c.r_off, c.q_ts, c.r_ts)[3])
        # a new query set drops the query table
        qf = np.zeros((int(c.q_off[-1]), 4), np.float32)
        _lib.check(L.vsc_tn_set_queries(c.h, qf.ctypes.data, c.q_off.ctypes.data, len(c.q_off) - 1, _lib.MEM_HOST))
        assert _run(c, table, 160, False)[0] == _lib.VSC_ERR_INVALID
    finally:
        c.close()


# ------------------------------------------------------------------------------------------- the localisers

def _video(rng, L, d, cls, vid, ts):
    x = rng.standard_normal((L, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return cls(video_id=vid, timestamps=ts(L), feature=x)


def _pairs_ts(dtype):
    return lambda L: np.stack([np.arange(L) / 3.0, (np.arange(L) + 1) / 3.0], axis=1).astype(dtype)


def planted_set(ts_q=None, ts_r=None, long_pair=False, d=128):
    """8 x 9 videos of 20..80 frames with four planted copies; long_pair: + a 100-frame query that is a copy of a
    100-frame reference (more cells than the DTW / DP kernels hold)."""
    from vsc2022_amd.vsc.index import VideoFeature

    rng = np.random.default_rng(7)
    ts_q = ts_q or (lambda k: _pairs_ts(np.float32))
    ts_r = ts_r or (lambda k: _pairs_ts(np.float32))
    queries = [_video(rng, int(rng.integers(20, 61)), d, VideoFeature, f"Q{k:06d}", ts_q(k)) for k in range(8)]
    refs = [_video(rng, int(rng.integers(25, 81)), d, VideoFeature, f"R{k:06d}", ts_r(k)) for k in range(9)]
    for qi, ri, q0, r0, L in [(0, 1, 2, 3, 15), (3, 3, 5, 10, 12), (5, 7, 10, 0, 10), (6, 2, 0, 12, 18)]:
        q, r = queries[qi], refs[ri]
        L = min(L, len(q) - q0, len(r) - r0)
        seg = r.feature[r0:r0 + L] + 0.05 * rng.standard_normal((L, d)).astype(np.float32)
        q.feature[q0:q0 + L] = seg / np.linalg.norm(seg, axis=1, keepdims=True)
    if long_pair:
        refs.append(_video(rng, 100, d, VideoFeature, "R000100", ts_r(9)))
        queries.append(VideoFeature(video_id="Q000100", timestamps=ts_q(8)(100), feature=refs[-1].feature.copy()))
    return queries, refs


def _candidates(queries, refs):
    from vsc2022_amd.vsc.metrics import CandidatePair

    return [CandidatePair(q.video_id, r.video_id, 0.25 + 0.01 * k) for k, (q, r) in enumerate(itertools.product(queries, refs))]


def _csv(write, *args):
    buf = io.StringIO()
    write(*args, buf)
    return buf.getvalue()


def _score_bits(matches):
    return [int(np.float32(m.score).view(np.uint32)) for m in matches]


def _check_table(loc, cands, min_pairs=2, same_types=True):
    """localize_table(c) is localize_all(c): tuples, score bits, value types, CSV bytes; pair / boxes describe the rows."""
    from vsc2022_amd.vsc.metrics import Match

    want = loc.localize_all(cands)
    table = loc.localize_table(cands)
    got = table.to_matches()
    assert got == want
    assert _score_bits(got) == _score_bits(want)
    if same_types:  # every value is the numpy scalar the per-box route yields (a Python float: its float64)
        assert [tuple(type(v) for v in m) for m in got] == [tuple(np.float64 if type(v) is float else type(v) for v in m) for m in want]
    assert _csv(table.write_csv) == _csv(Match.write_csv, want)
    assert len({(m.query_id, m.ref_id) for m in want}) >= min_pairs  # not vacuous
    assert [(cands[k].query_id, cands[k].ref_id) for k in table.pair] == [(m.query_id, m.ref_id) for m in want]
    assert (np.diff(table.pair) >= 0).all() and table.boxes.shape == (len(want), 4)
    for m, (x1, y1, x2, y2) in zip(want, table.boxes.tolist()):
        q, r = loc.queries[m.query_id], loc.refs[m.ref_id]
        assert (q.get_timestamps(x1)[0], q.get_timestamps(x2)[1], r.get_timestamps(y1)[0], r.get_timestamps(y2)[1]) == m[3:]
    return table, want


TN_KW = dict(model_type="TN", tn_max_step=5, min_length=4)


def _localisers():
    from vsc2022_amd.vsc.baseline import localization as loc

    return {"base": (loc.VCSLLocalization, 0.0), "maxsim": (loc.VCSLLocalizationMaxSim, 0.5),
            "candscore": (loc.VCSLLocalizationCandidateScore, 0.0)}


@pytest.mark.parametrize("which", ["base", "maxsim", "candscore"])
def test_localize_table_tn(gpu, which):
    cls, bias = _localisers()[which]
    queries, refs = planted_set()
    aligner = cls(queries, refs, similarity_bias=bias, **TN_KW)
    assert aligner._can_fuse()
    cands = _candidates(queries, refs)
    table, want = _check_table(aligner, cands)
    assert table.score.dtype == (np.float32 if which == "maxsim" else np.float64)
    assert table.query_start.dtype == np.float32
    # a batch split in two and concatenated is the same table
    from vsc2022_amd.vsc.metrics import MatchTable

    halves = MatchTable.concat([aligner.localize_table(cands[:31]), aligner.localize_table(cands[31:])], pair_offsets=[0, 31])
    assert halves.to_matches() == want and halves.pair.tolist() == table.pair.tolist()
    assert np.array_equal(halves.boxes, table.boxes) and halves.score.dtype == table.score.dtype
    assert aligner.localize_table([]).to_matches() == [] and len(aligner.localize_table(cands[:1])) == len(aligner.localize_all(cands[:1]))


@pytest.mark.parametrize("which", ["maxsim", "candscore"])
@pytest.mark.parametrize("name", ["DTW", "DP"])
def test_localize_table_device_aligners_with_a_spliced_pair(gpu, name, which):
    from vsc2022_amd import _lib

    cls, bias = _localisers()[which]
    queries, refs = planted_set(long_pair=True)
    aligner = cls(queries, refs, name, similarity_bias=bias, on_device=True, min_sim=0.5 + bias, min_length=4)
    assert aligner._can_fuse_align() and 100 * 100 > _lib.ALIGN_MAX_CELLS
    cands = _candidates(queries, refs)
    cands.insert(5, cands.pop())  # the long pair (last of the product) goes between ordinary ones
    status = aligner._aligned_boxes(cands)[3]
    long_k = [k for k, c in enumerate(cands) if (c.query_id, c.ref_id) == ("Q000100", "R000100")]
    assert list(np.flatnonzero(status)) == long_k  # the one pair the kernel hands back
    table, want = _check_table(aligner, cands, min_pairs=3)
    assert long_k == [5] and 5 in table.pair.tolist() and table.pair.max() > 5  # spliced in, not appended
    assert any((m.query_id, m.ref_id) == ("Q000100", "R000100") for m in want)


def test_localize_table_host_routes(gpu):
    """HV (host aligner) and a subclass with its own score(): the table is assembled on the host from the same rows."""
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim

    queries, refs = planted_set()
    cands = _candidates(queries, refs)
    hv = VCSLLocalizationMaxSim(queries, refs, "HV", min_sim=0.5, min_length=4)
    assert not hv._can_fuse() and not hv._can_fuse_align()
    _check_table(hv, cands)

    class BoxMean(VCSLLocalizationMaxSim):
        def score(self, candidate, match, box, similarity):
            x1, y1, x2, y2 = box
            return float(similarity[x1:x2 + 1, y1:y2 + 1].mean())

    own = BoxMean(queries, refs, similarity_bias=0.5, **TN_KW)
    assert not own._can_fuse()
    table, _ = _check_table(own, cands)
    assert table.score.dtype == np.float64


def test_one_dimensional_and_mixed_timestamps(gpu):
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim

    # 1-D integer timestamps on the query side; on the reference side float32 and float64 pairs alternate, so that the
    # matched references disagree in dtype
    queries, refs = planted_set(ts_q=lambda k: (lambda L: np.arange(L, dtype=np.int64) * 40),
                                ts_r=lambda k: _pairs_ts(np.float32 if k % 2 else np.float64))
    aligner = VCSLLocalizationMaxSim(queries, refs, similarity_bias=0.5, **TN_KW)
    table, want = _check_table(aligner, _candidates(queries, refs), same_types=False)  # (one column, one dtype)
    assert table.query_start.dtype == np.int64 and table.ref_start.dtype == np.float64
    assert {type(m.ref_start) for m in want} == {np.float32, np.float64}
    # ... and with only float32 references among the matched ones the column stays float32
    only = [c for c in _candidates(queries, refs) if int(c.ref_id[1:]) % 2]
    table, _ = _check_table(aligner, only)
    assert table.ref_start.dtype == np.float32


@pytest.mark.parametrize("case", ["g5_localization_default", "g5_localization_ref_params", "g5_localization_ref_params_nobias"])
def test_goldens_through_localize_table(gpu, case):
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationCandidateScore, VCSLLocalizationMaxSim
    from vsc2022_amd.vsc.index import VideoFeature
    from vsc2022_amd.vsc.metrics import CandidatePair

    fx = load(case)
    kw = {str(k): int(v) for k, v in zip(fx["kw_keys"], fx["kw_vals"])}
    bias = float(fx["bias"])
    q, r = videos(fx, "q", VideoFeature), videos(fx, "r", VideoFeature)
    cands = [CandidatePair(str(a), str(b), float(s)) for a, b, s in zip(fx["cand_q"], fx["cand_r"], fx["cand_s"])]
    for cls, tag, extra in ((VCSLLocalizationMaxSim, "maxsim", dict(similarity_bias=bias)), (VCSLLocalizationCandidateScore, "candscore", {})):
        aligner = cls(q, r, "TN", **extra, **kw)
        table = aligner.localize_table(cands)
        exp = fx[f"{tag}_m_rows"]
        assert len(table) == len(exp)
        assert list(table.query_id) == list(fx[f"{tag}_m_q"]) and list(table.ref_id) == list(fx[f"{tag}_m_r"])
        got = np.stack([table.query_start, table.query_end, table.ref_start, table.ref_end], axis=1).astype(np.float64)
        assert np.array_equal(got, exp[:, 1:])
        assert np.allclose(table.score, exp[:, 0], atol=2e-6)  # the fixture's np.matmul round-off, as for localize_all
        want = aligner.localize_all(cands)
        assert table.to_matches() == want and _score_bits(table.to_matches()) == _score_bits(want)


@functools.lru_cache(maxsize=None)
def _g8():
    from vsc2022_amd import synth
    from vsc2022_amd.vsc.index import VideoFeature

    return tuple(synth.to_video_features(v, VideoFeature) for v in g8_inputs()[:3])


@pytest.mark.parametrize("score_normalization", [False, True])
def test_sscd_localize_table_writes_the_same_file(gpu, score_normalization):
    from vsc2022_amd.vsc.baseline import sscd_baseline as sb
    from vsc2022_amd.vsc.baseline.score_normalization import score_normalize
    from vsc2022_amd.vsc.metrics import Match

    queries, refs, noise = _g8()
    if score_normalization:
        queries, refs = score_normalize(queries, refs, noise, beta=sb.CONSTANTS.score_norm_beta)
    pairs = sb.search(queries, refs)
    want = sb.localize_and_verify(queries, refs, pairs, score_normalization=score_normalization)
    table = sb.localize_table(queries, refs, pairs, score_normalization=score_normalization)
    assert len(want) >= 10 and table.to_matches() == want
    assert _csv(table.write_csv) == _csv(Match.write_csv, want)
    assert len(sb.localize_table(queries, refs, pairs, localize_per_query=0.1).pair) <= len(table)


# ------------------------------------------------------------------------------------------- the engine

def _flat(videos_):
    from vsc2022_amd.vsc.index import VideoLayout

    layout = VideoLayout(videos_)
    return VideoLayout.features(videos_), layout.offsets, np.concatenate([v.timestamps for v in videos_], axis=0), layout.video_ids


@pytest.mark.parametrize("box_score", ["maxsim", "candidate"])
def test_engine_rows_are_the_stock_localisers(gpu, box_score):
    from vsc2022_amd import engine
    from vsc2022_amd.vsc.baseline import sscd_baseline as sb
    from vsc2022_amd.vsc.baseline.score_normalization import score_normalize
    from vsc2022_amd.vsc.candidates import CandidateList

    queries, refs, noise = _g8()
    normalised = box_score == "maxsim"
    if normalised:
        queries, refs = score_normalize(queries, refs, noise, beta=sb.CONSTANTS.score_norm_beta)
    bias = sb.CONSTANTS.score_norm_bias if normalised else 0.0
    (qf, q_off, q_ts, q_ids), (rf, r_off, r_ts, r_ids) = _flat(queries), _flat(refs)
    m = engine.DeviceMatcher(rf, r_off, r_ts=r_ts)
    m.set_queries(qf, q_off, q_ts=q_ts)
    plain = m.match(bias=bias)
    arrays = ("cand_q", "cand_r", "cand_score", "loc_index", "nbox", "boxes", "box_score")
    before = {f: getattr(plain, f).cpu().numpy().copy() for f in arrays}  # (the result's tensors are the matcher's buffers)
    res = m.match(bias=bias, rows=True, box_score=box_score)
    # the default result is what it was: same fields, no rows
    assert plain.row_cand is None and plain.row_times is None
    for f in ("n_hits", "n_pairs", "n_candidates", "n_localized", "n_matches", "radius"):
        assert getattr(plain, f) == getattr(res, f)
    n_loc = res.n_localized
    for f in arrays:
        a, b = before[f], getattr(res, f).cpu().numpy()
        if f in ("boxes", "box_score"):  # (only the slots below nbox are defined)
            live = np.arange(16)[None, :] < before["nbox"][:, None]
            a, b = a[live], b[live]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f
    assert res.row_times.dtype.is_floating_point and res.row_times.element_size() == 8 and res.row_times.shape == (res.n_matches, 4)
    table = m.match_table(res, q_ids, r_ids)
    # the stock localiser over the same candidate prefix, on the same descriptors
    n = res.n_localized
    cands = CandidateList(res.cand_q[:n].cpu().numpy(), res.cand_r[:n].cpu().numpy(), res.cand_score[:n].cpu().numpy(), q_ids, r_ids)
    aligner = sb._aligner(queries, refs, normalised) if normalised else \
        sb.loc.VCSLLocalizationCandidateScore(queries, refs, **TN_KW)
    want = aligner.localize_all(cands)
    assert len(want) == res.n_matches >= 10
    got = table.to_matches()
    assert got == want and _score_bits(got) == _score_bits(want)
    assert table.pair.tolist() == res.row_cand.cpu().tolist() and table.query_start.dtype == q_ts.dtype
    assert _csv(table.write_csv) == _csv(sb.M.Match.write_csv, want)
    if box_score == "candidate":
        return
    # a second query set on the same matcher: the new set's rows; without q_ts, rows=True is refused
    half = queries[: len(queries) // 2][::-1]
    hf, h_off, h_ts, h_ids = _flat(half)
    m.set_queries(hf, h_off, q_ts=h_ts + 1000.0)
    res2 = m.match(bias=bias, rows=True)
    cands2 = CandidateList(res2.cand_q[:res2.n_localized].cpu().numpy(), res2.cand_r[:res2.n_localized].cpu().numpy(),
                           res2.cand_score[:res2.n_localized].cpu().numpy(), h_ids, r_ids)
    shifted = [type(v)(video_id=v.video_id, timestamps=v.timestamps + 1000.0, feature=v.feature) for v in half]
    want2 = sb._aligner(shifted, refs, True).localize_all(cands2)
    assert len(want2) >= 5 and m.match_table(res2, h_ids, r_ids).to_matches() == want2
    m.set_queries(hf, h_off)
    with pytest.raises(ValueError, match="timestamps"):
        m.match(bias=bias, rows=True)
    assert m.match(bias=bias).n_matches == res2.n_matches
