"""The pair aggregation (include/vscmi.h, vsc_pair_aggregate) restated with a Python dict and explicit float64 loops,
sharing no code with the product.  Not a test module.

Per (query video, ref video) pair, in first-appearance order over the hit list (a dict keeps insertion order): d = the
pair's fp32 scores as Python floats (float64), `sorted(..., reverse=True)`;
    max      the largest score (a run holding both zeros: +0.0, as the header says);
    sum      acc = 0.0; for v in d: acc = acc + v;  float32(acc)
    mean     float32(acc / float(c))
    topmean  the same loop over d[:min(m, c)], / float(min(m, c))
then the pairs stably sorted by the fp32 result, descending (Python's sort: -0.0 == +0.0, equal keys keep their order).
"""
import math

import numpy as np


def aggregate_run(scores, agg, m=1):
    """One pair: `scores` its fp32 hit scores in any order; agg "max" | "sum" | "mean" | "topmean"."""
    d = sorted((float(np.float32(v)) for v in scores), reverse=True)
    if agg == "max":
        top = d[0]
        if top == 0.0:  # both zeros compare equal: +0.0 wins where the run holds one
            top = 0.0 if any(v == 0.0 and math.copysign(1.0, v) > 0 for v in d) else -0.0
        return np.float32(top)
    k = min(int(m), len(d)) if agg == "topmean" else len(d)
    acc = 0.0
    for v in d[:k]:
        acc = acc + v
    with np.errstate(over="ignore"):
        if agg == "sum":
            return np.float32(acc)
        if agg in ("mean", "topmean"):
            return np.float32(acc / float(k))
    raise ValueError(agg)


def pair_aggregate_ref(i, j, s, row2q, row2r, agg, m=1):
    """Columns (q int32, r int32, score float32, first int64, count int32) of the candidate table of a hit list."""
    groups = {}
    for x in range(len(s)):
        key = (int(row2q[int(i[x])]), int(row2r[int(j[x])]))
        if key not in groups:
            groups[key] = (x, [])
        groups[key][1].append(s[x])
    rows = [(q, r, aggregate_run(vals, agg, m), first, len(vals)) for (q, r), (first, vals) in groups.items()]
    rows = sorted(rows, key=lambda t: float(t[2]), reverse=True)
    return (np.array([t[0] for t in rows], dtype=np.int32), np.array([t[1] for t in rows], dtype=np.int32),
            np.array([t[2] for t in rows], dtype=np.float32), np.array([t[3] for t in rows], dtype=np.int64),
            np.array([t[4] for t in rows], dtype=np.int32))


# ---- the hit lists tests/test_gpu_pair_agg.py and tests/test_gpu_lifetime.py run, and the comparison of the columns

ROWS_PER_VIDEO = 3


def hits(runs, seed):
    """runs: [(q video, r video, scores)] -> (i, j, s, row2q, row2r) in SEARCH order (score desc, row asc, ref asc);
    every video has ROWS_PER_VIDEO rows and a hit picks one of them at random."""
    rng = np.random.default_rng(seed)
    nqv = max(q for q, _, _ in runs) + 1
    nrv = max(r for _, r, _ in runs) + 1
    row2q = np.repeat(np.arange(nqv, dtype=np.int32), ROWS_PER_VIDEO)
    row2r = np.repeat(np.arange(nrv, dtype=np.int32), ROWS_PER_VIDEO)
    i = np.concatenate([q * ROWS_PER_VIDEO + rng.integers(0, ROWS_PER_VIDEO, len(sc)) for q, _, sc in runs]).astype(np.int32)
    j = np.concatenate([r * ROWS_PER_VIDEO + rng.integers(0, ROWS_PER_VIDEO, len(sc)) for _, r, sc in runs]).astype(np.int32)
    s = np.concatenate([np.asarray(sc, dtype=np.float32) for _, _, sc in runs])
    order = np.lexsort((j, i, -s.astype(np.float64)))
    return i[order], j[order], s[order], row2q, row2r


def case(name):
    rng = np.random.default_rng(100 + CASES.index(name))
    if name == "one_hit":
        runs = [(2, 1, [0.5])]
    elif name == "one_pair":
        runs = [(0, 0, rng.standard_normal(5000))]
    elif name == "run_lengths":
        # pairs in key order (q ascending): the sorted runs start at 0, 1, 64, 128, 193, 448, 704, 961 -- the runs of 256,
        # 257 and 1000 hits each lie across a multiple of 256 (checked below)
        lens = [1, 63, 64, 65, 255, 256, 257, 1000, 1, 63, 64, 65, 255, 256, 257, 1000]
        runs = [(q, int(rng.integers(0, 5)), rng.standard_normal(n)) for q, n in enumerate(lens)]
        starts = np.r_[0, np.cumsum(lens)]
        assert any(a // 256 != (b - 1) // 256 and a % 256 for a, b in zip(starts[:-1], starts[1:]))
    elif name == "distinct":
        pairs = rng.permutation(70 * 60)[:3000]
        runs = [(int(p // 60), int(p % 60), [v]) for p, v in zip(pairs, rng.standard_normal(3000))]
    elif name == "quantised":
        pair = rng.integers(0, 600, 20000)
        sc = rng.integers(-4, 5, 20000) / 8.0
        runs = [(int(p // 25), int(p % 25), sc[pair == p]) for p in np.unique(pair)]
    elif name == "order_revealing":
        runs = [(int(p // 8), int(p % 8), rng.standard_normal(int(rng.integers(1, 40)))) for p in range(50)]
        runs += [(7, 0, [2.0 ** 53] + [1.0] * 64 + [-(2.0 ** 53)]), (7, 1, [1e30, -1e30, 1.0]),
                 (7, 2, [2.0 ** 53] + [1.0] * 300 + [-(2.0 ** 53)]), (7, 3, [1.0, 1e30, -1e30, 0.25])]
    else:
        raise KeyError(name)
    return hits(runs, len(name))


CASES = ["one_hit", "one_pair", "run_lengths", "distinct", "quantised", "order_revealing"]


def assert_columns(got, exp, what):
    from helpers import bits

    names = ("q", "r", "score", "first", "count")
    assert len(got[0]) == len(exp[0]), (what, len(got[0]), len(exp[0]))
    for name, g, e in zip(names, got, exp):
        if name == "score":
            bad = np.flatnonzero(bits(g) != bits(e))
        else:
            bad = np.flatnonzero(g != e)
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), e[bad[:5]].tolist())
