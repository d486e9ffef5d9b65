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
