"""The match-rows stage (include/vscmi.h, vsc_tn_match_rows) restated in numpy, and the synthetic box tables the CPU
and GPU tests share.  Not a test module."""
import numpy as np

MAX_BOXES = 16


def rows(pair_q, pair_r, nbox, boxes, boxmax, q_off, r_off, q_ts, r_ts):
    """(pair int32 [n], box int32 [n, 4], score fp32 [n], times float64 [n, 4]) in (pair, box slot) order."""
    nbox = np.asarray(nbox, dtype=np.int64)
    pair = np.repeat(np.arange(len(nbox), dtype=np.int64), nbox)
    slot = np.arange(int(nbox.sum()), dtype=np.int64) - np.repeat(np.cumsum(nbox) - nbox, nbox)
    box = np.asarray(boxes).reshape(-1, MAX_BOXES, 4)[pair, slot]
    score = np.asarray(boxmax).reshape(-1, MAX_BOXES)[pair, slot]
    q0, r0 = np.asarray(q_off)[np.asarray(pair_q)[pair]], np.asarray(r_off)[np.asarray(pair_r)[pair]]
    times = np.stack([q_ts[q0 + box[:, 0], 0], q_ts[q0 + box[:, 2], 1], r_ts[r0 + box[:, 1], 0], r_ts[r0 + box[:, 3], 1]], axis=1)
    return pair.astype(np.int32), box.astype(np.int32), score.astype(np.float32), times.astype(np.float64).reshape(-1, 4)


def video_tables(seed=5, n_q=40, n_r=50, max_len=70):
    """(q_off, r_off, q_ts, r_ts): 40 query / 50 reference videos of 0..70 frames (zero-length videos included) and
    float64 [rows, 2] timestamps that float32 cannot hold (k / 3)."""
    rng = np.random.default_rng(seed)
    q_len, r_len = rng.integers(0, max_len + 1, n_q), rng.integers(0, max_len + 1, n_r)
    q_len[[3, n_q - 1]] = 0
    r_len[[0, 7]] = 0
    q_len[5], r_len[5] = max_len, 1
    q_off, r_off = np.r_[0, np.cumsum(q_len)].astype(np.int64), np.r_[0, np.cumsum(r_len)].astype(np.int64)
    q_ts = (np.arange(2 * q_off[-1], dtype=np.float64) / 3.0).reshape(-1, 2)
    r_ts = (1000.0 + np.arange(2 * r_off[-1], dtype=np.float64) / 3.0).reshape(-1, 2)
    assert (q_ts.astype(np.float32).astype(np.float64) != q_ts).any()
    return q_off, r_off, q_ts, r_ts


PATTERNS = ("zeros", "full", "uniform", "last", "first")


def box_table(n_pairs, pattern, q_off, r_off, seed=0):
    """(pair_q, pair_r, nbox, boxes, boxmax) of n_pairs pairs (repeats included).  Pairs with an empty video have no
    boxes; everywhere else the corners are random frames of the pair's videos, frame 0 and frame L - 1 among them.  The
    slots beyond nbox hold corners far outside every video: nothing may read through them."""
    rng = np.random.default_rng(seed + 1000 * PATTERNS.index(pattern) + n_pairs)
    n_q, n_r = len(q_off) - 1, len(r_off) - 1
    pair_q = rng.integers(0, n_q, n_pairs).astype(np.int32)
    pair_r = rng.integers(0, n_r, n_pairs).astype(np.int32)
    if n_pairs > 2:
        pair_q[1], pair_r[1] = pair_q[0], pair_r[0]  # a repeated pair
    lq, lr = np.diff(q_off)[pair_q], np.diff(r_off)[pair_r]
    usable = (lq > 0) & (lr > 0)
    if n_pairs and pattern in ("last", "first", "full"):  # the pairs these patterns are about must be able to hold boxes
        fix = {"last": [n_pairs - 1], "first": [0], "full": range(n_pairs)}[pattern]
        good_q, good_r = np.flatnonzero(np.diff(q_off) > 0), np.flatnonzero(np.diff(r_off) > 0)
        for p in fix:
            if not usable[p]:
                pair_q[p], pair_r[p] = good_q[p % len(good_q)], good_r[p % len(good_r)]
        lq, lr = np.diff(q_off)[pair_q], np.diff(r_off)[pair_r]
        usable = (lq > 0) & (lr > 0)
    nbox = {"zeros": np.zeros(n_pairs), "full": np.full(n_pairs, MAX_BOXES), "uniform": rng.integers(0, MAX_BOXES + 1, n_pairs),
            "last": np.r_[np.zeros(max(n_pairs - 1, 0)), [7][:n_pairs]], "first": np.r_[[9][:n_pairs], np.zeros(max(n_pairs - 1, 0))],
            }[pattern].astype(np.int32)
    nbox[~usable] = 0
    boxes = np.full((n_pairs, MAX_BOXES, 4), 1 << 30, dtype=np.int32)
    u = rng.random((n_pairs, MAX_BOXES, 4))
    span = np.stack([lq, lr, lq, lr], axis=-1)[:, None, :].astype(np.float64)
    corners = np.minimum((u * span).astype(np.int64), np.maximum(span.astype(np.int64) - 1, 0))
    corners[:, 0] = 0                                              # slot 0: frame 0 ...
    corners[:, 1] = np.maximum(span.astype(np.int64)[:, 0] - 1, 0)  # slot 1: ... and frame L - 1 of both sides
    live = np.arange(MAX_BOXES)[None, :] < nbox[:, None]
    boxes[live] = corners[live]
    boxmax = rng.standard_normal((n_pairs, MAX_BOXES)).astype(np.float32)
    boxmax[:, 3] = -np.inf  # (an empty slice scores -inf: bits are copied, not compared)
    return pair_q, pair_r, nbox, boxes, boxmax
