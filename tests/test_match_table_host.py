"""Host side of the match-rows stage: `vsc.metrics.MatchTable` (columns <-> Match tuples <-> CSV bytes), the numpy
restatement of the stage the GPU tests compare the kernels against, the two C-ABI names, and what the entry point rejects
before any device is needed."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import match_rows_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csv(write, *args):
    buf = io.StringIO()
    write(*args, buf)
    return buf.getvalue()


def _table(score_dtype, ts):
    """A hand-made table over two query / two reference videos with `ts(L)` timestamps, built the way the scalar route
    builds its rows (get_timestamps of the box corners)."""
    from vsc2022_amd.vsc.index import VideoMetadata
    from vsc2022_amd.vsc.metrics import Match, MatchTable

    q = {"Q000001": VideoMetadata("Q000001", ts(9)), "Q000002": VideoMetadata("Q000002", ts(30))}
    r = {"R000007": VideoMetadata("R000007", ts(12)), "R000008": VideoMetadata("R000008", ts(5))}
    rows = [("Q000001", "R000007", 0.1, (0, 3, 8, 11)), ("Q000001", "R000007", 0.7, (2, 0, 5, 4)),
            ("Q000002", "R000008", 1.0 / 3.0, (29, 4, 29, 4)), ("Q000002", "R000007", -0.25, (1, 1, 20, 10))]
    want = [Match(qi, ri, score_dtype(s), q[qi].get_timestamps(x1)[0], q[qi].get_timestamps(x2)[1],
                  r[ri].get_timestamps(y1)[0], r[ri].get_timestamps(y2)[1]) for qi, ri, s, (x1, y1, x2, y2) in rows]
    table = MatchTable.from_matches(want, pair=[0, 0, 1, 2], boxes=[b for *_, b in rows])
    return table, want


TS = {
    "f32_pairs": lambda L: np.stack([np.arange(L) / 3.0, (np.arange(L) + 1) / 3.0], axis=1).astype(np.float32),
    "f64_pairs": lambda L: np.stack([np.arange(L) / 3.0, (np.arange(L) + 1) / 3.0], axis=1),
    "int_1d": lambda L: np.arange(L, dtype=np.int64) * 2,
}


@pytest.mark.parametrize("score_dtype", [np.float32, np.float64, float])
@pytest.mark.parametrize("ts", sorted(TS))
def test_round_trip_and_csv_bytes(ts, score_dtype):
    from vsc2022_amd.vsc.metrics import Match

    table, want = _table(score_dtype, TS[ts])
    assert len(table) == 4
    got = table.to_matches()
    assert got == want
    assert [type(m.query_start) for m in got] == [type(m.query_start) for m in want]
    text = _csv(table.write_csv)
    assert text == _csv(Match.write_csv, want) == _csv(Match.write_csv, got)
    assert text.splitlines()[0] == "query_id,ref_id,score,query_start,query_end,ref_start,ref_end" and len(text.splitlines()) == 5
    assert table.score.dtype == (np.float32 if score_dtype is np.float32 else np.float64)
    assert table.query_start.dtype == TS[ts](1).dtype
    assert table.pair.tolist() == [0, 0, 1, 2] and table.boxes.shape == (4, 4) and table.boxes.dtype == np.int32


def test_empty_table_writes_the_header_only():
    from vsc2022_amd.vsc.metrics import Match, MatchTable

    for table in (MatchTable.empty(), MatchTable.from_matches([]), MatchTable.empty(np.float32, np.float32)):
        assert len(table) == 0 and table.to_matches() == []
        assert _csv(table.write_csv) == _csv(Match.write_csv, []) == "query_id,ref_id,score,query_start,query_end,ref_start,ref_end\n"


def test_concatenation_keeps_order_and_dtypes():
    from vsc2022_amd.vsc.metrics import Match, MatchTable

    a, want_a = _table(np.float32, TS["f32_pairs"])
    b, want_b = _table(np.float32, TS["f32_pairs"])
    both = MatchTable.concat([a, MatchTable.empty(), b], pair_offsets=[0, 3, 3])
    assert both.to_matches() == want_a + want_b and (a + b).to_matches() == want_a + want_b
    assert both.score.dtype == np.float32 and both.query_end.dtype == np.float32  # (the empty float64 table does not vote)
    assert both.pair.tolist() == [0, 0, 1, 2, 3, 3, 4, 5] and both.boxes.shape == (8, 4)
    assert _csv(both.write_csv) == _csv(Match.write_csv, want_a + want_b)
    # float32 rows followed by float64 rows: the column is float64, as a list of those scalars becomes
    c, want_c = _table(np.float64, TS["f64_pairs"])
    mixed = a + c
    assert mixed.score.dtype == np.float64 and mixed.ref_start.dtype == np.float64
    assert _csv(mixed.write_csv) == _csv(Match.write_csv, want_a + want_c)
    assert len(MatchTable.concat([])) == 0
    picked = both.take(np.array([5, 0]))
    assert picked.to_matches() == [want_b[1], want_a[0]]


@pytest.mark.parametrize("pattern", mr.PATTERNS)
@pytest.mark.parametrize("n_pairs", [0, 1, 37, 300])
def test_restatement_is_the_scalar_route(n_pairs, pattern):
    """np.repeat / cumsum / fancy indexing against the per-box loop of VCSLLocalization.localize_all."""
    q_off, r_off, q_ts, r_ts = mr.video_tables()
    pair_q, pair_r, nbox, boxes, boxmax = mr.box_table(n_pairs, pattern, q_off, r_off)
    pair, box, score, times = mr.rows(pair_q, pair_r, nbox, boxes, boxmax, q_off, r_off, q_ts, r_ts)
    want = []
    for k in range(n_pairs):
        tq, tr = q_ts[q_off[pair_q[k]]:q_off[pair_q[k] + 1]], r_ts[r_off[pair_r[k]]:r_off[pair_r[k] + 1]]
        for b in range(int(nbox[k])):
            x1, y1, x2, y2 = (int(v) for v in boxes[k, b])
            want.append((k, (x1, y1, x2, y2), boxmax[k, b], (tq[x1][0], tq[x2][1], tr[y1][0], tr[y2][1])))
    assert len(want) == len(pair) == int(nbox.sum())
    assert pair.tolist() == [w[0] for w in want] and [tuple(b) for b in box.tolist()] == [w[1] for w in want]
    assert score.view(np.uint32).tolist() == [int(np.float32(w[2]).view(np.uint32)) for w in want]
    assert [tuple(t) for t in times.tolist()] == [tuple(float(v) for v in w[3]) for w in want]
    if pattern == "full" and n_pairs:
        assert len(pair) == 16 * n_pairs and (box[:, 0] == 0).any() and (box == 1 << 30).sum() == 0
    if pattern in ("last", "first") and n_pairs:
        assert len(pair) in (7, 9)


def test_header_exports_and_argtypes():
    from vsc2022_amd import _lib

    header = open(os.path.join(ROOT, "include", "vscmi.h")).read()
    declared = set(re.findall(r"\b(vsc_[a-z0-9_]+)\s*\(", header))
    for name in ("vsc_tn_set_timestamps", "vsc_tn_match_rows"):
        assert name in declared and name in _lib.EXPORTS
    L = _lib.lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert L.vsc_tn_set_timestamps.argtypes == [vp, vp, vp, i32]
    assert L.vsc_tn_match_rows.argtypes == [vp, vp, vp, i64, i32, vp, vp, vp, i32, vp, vp, vp, vp, i64, i32, ctypes.POINTER(i64)]
    assert L.vsc_tn_match_rows.restype is ctypes.c_int
    # the accounting class of the rows launches exists; the one after it does not
    ms, n, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    assert L.vsc_aux_profile_read(3, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(by), 0) == _lib.VSC_OK
    assert L.vsc_aux_profile_read(4, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(by), 0) == _lib.VSC_ERR_INVALID


def _call(pair_q, pair_r, nbox, boxes, boxmax, cap=64, ctx=None):
    from vsc2022_amd import _lib

    out_pair, out_box = np.full(cap, -7, np.int32), np.full((cap, 4), -7, np.int32)
    out_score, out_times = np.full(cap, -7, np.float32), np.full((cap, 4), -7, np.float64)
    n_rows = ctypes.c_int64(-1)
    rc = _lib.lib().vsc_tn_match_rows(ctx, pair_q.ctypes.data, pair_r.ctypes.data, len(pair_q), _lib.MEM_HOST, nbox.ctypes.data,
                                      boxes.ctypes.data, boxmax.ctypes.data, _lib.MEM_HOST, out_pair.ctypes.data,
                                      out_box.ctypes.data, out_score.ctypes.data, out_times.ctypes.data, cap, _lib.MEM_HOST,
                                      ctypes.byref(n_rows))
    untouched = (out_pair == -7).all() and (out_box == -7).all() and (out_score == -7).all() and (out_times == -7).all()
    return rc, untouched


@pytest.mark.parametrize("bad, says", [(dict(nbox=17), "box count"), (dict(nbox=-1), "box count"),
                                       (dict(corner=-1), "negative box corner"), (dict(pair_q=-1), "ordinal"),
                                       (dict(pair_r=-3), "ordinal"), (dict(), "no context")])
def test_rejected_inputs_at_the_c_abi(bad, says):
    """Host-memory inputs: VSC_ERR_INVALID before any device is touched (no context exists here); the message names what
    was found, so each case is refused for its own reason.  The checks that need the videos' lengths (a corner equal to
    the length, an ordinal beyond the last video) are in tests/test_gpu_match_rows.py."""
    from vsc2022_amd import _lib

    pair_q, pair_r = np.array([0, 1, 2], np.int32), np.array([2, 1, 0], np.int32)
    nbox = np.array([1, 2, 0], np.int32)
    boxes = np.zeros((3, 16, 4), np.int32)
    boxes[:, 2:] = -5  # (slots beyond nbox are not looked at)
    boxmax = np.zeros((3, 16), np.float32)
    if "nbox" in bad:
        nbox[1] = bad["nbox"]
    if "corner" in bad:
        boxes[1, 1, 3] = bad["corner"]
    if "pair_q" in bad:
        pair_q[2] = bad["pair_q"]
    if "pair_r" in bad:
        pair_r[0] = bad["pair_r"]
    rc, untouched = _call(pair_q, pair_r, nbox, boxes, boxmax)
    assert rc == _lib.VSC_ERR_INVALID and untouched
    assert says in _lib.lib().vsc_last_error().decode()
    with pytest.raises(ValueError):
        _lib.check(rc)
    assert _lib.lib().vsc_tn_set_timestamps(None, None, None, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID


def test_rows_without_timestamps_is_a_value_error():
    """DeviceMatcher.match(rows=True) asks for the timestamps before it does anything else."""
    from vsc2022_amd import engine

    m = object.__new__(engine.DeviceMatcher)
    with pytest.raises(ValueError, match="timestamps"):
        m.match(rows=True)
    m._q_ts = m._r_ts = None
    with pytest.raises(ValueError, match="timestamps"):
        m.match(rows=True)
    with pytest.raises(ValueError, match="box_score"):
        m.match(box_score="mean")
