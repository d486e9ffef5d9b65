"""The CPU oracle and the input classes of tests/chain_cases.py are what they claim to be (no GPU).

* The oracle's chains (`orc.scores`, `orc.pair_sims`, `orc.row_normalize`) against an exact restatement in Python integers:
  every fp32 value is an integer multiple of 2^-149, a step `q r + acc` is computed exactly on the 2^-298 grid and rounded
  ONCE to float32, to nearest-even, with gradual underflow and overflow to inf.  It shares no code with the oracle and
  uses no floating-point arithmetic, so a process with DAZ / FTZ set, or a compiler that contracted, reordered or
  vectorised the oracle's loop differently, shows as a difference in bits.
* Discriminating power: the same restatement with one fault switched on -- operands flushed, results flushed, the
  product rounded before the addition, k descending -- must differ in bits from the oracle on at least a quarter of the
  pairs of the class aimed at that fault.  A quarter is a floor that keeps a class from testing nothing, not a tolerance.
* The shares of +0.0 / -0.0 / +inf / -inf / NaN results the classes promise, and that the thresholds of the searches in
  tests/test_gpu_chain_contract.py cut where they are meant to.
"""
import math

import numpy as np
import pytest

import chain_cases as cc

U = 149           # fp32 values are integers in units of 2^-U
INF, NINF, NAN = "inf", "-inf", "nan"


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- exact restatement (integers only)
def to_units(x):
    """float32 -> (value in units of 2^-149 as a Python int | INF | NINF | NAN, sign bit): read from the bit pattern"""
    b = int(np.float32(x).view(np.uint32))
    neg, e, m = b >> 31, (b >> 23) & 0xFF, b & 0x7FFFFF
    if e == 255:
        return (NAN if m else (NINF if neg else INF)), neg
    v = m if e == 0 else (m | 0x800000) << (e - 1)
    return (-v if neg else v), neg


def round_units(n, scale):
    """n 2^-scale (n a non-zero int, scale >= U) rounded to float32, nearest-even, gradual underflow:
    (value in units of 2^-149 | INF | NINF), or 0 with the sign of n when it underflows to zero."""
    neg, a = n < 0, abs(n)
    drop = max(a.bit_length() - 24, scale - U)         # bits below the 24-bit significand, or below 2^-149
    if drop > 0:
        keep, rem, half = a >> drop, a & ((1 << drop) - 1), 1 << (drop - 1)
        if rem > half or (rem == half and (keep & 1)):
            keep += 1
    else:
        keep = a << -drop
    # keep 2^(drop - scale); the largest finite float32 is (2^24 - 1) 2^104
    if keep.bit_length() + drop - scale > 128:
        return NINF if neg else INF
    v = keep << (drop - (scale - U))
    return -v if neg else v


def to_f32(v, neg_zero=False):
    if v == INF:
        return np.float32(np.inf)
    if v == NINF:
        return np.float32(-np.inf)
    if v == NAN:
        return np.float32(np.nan)
    if v == 0:
        return np.float32(-0.0 if neg_zero else 0.0)
    return np.float32(math.ldexp(v, -U))           # (exact: |v| has at most 24 significant bits)


def _flush(v):
    return 0 if isinstance(v, int) and abs(v) < (1 << 23) else v      # |x| < 2^-126 -> 0 (the sign is kept by the caller)


def fma_step(a, a_neg, b, b_neg, acc, acc_neg, unfused=False, flush_out=False):
    """(acc, sign bit of acc) after acc = fmaf(a, b, acc); every value as to_units gives it"""
    if NAN in (a, b, acc):
        return NAN, 0
    p_neg = a_neg ^ b_neg
    if a in (INF, NINF) or b in (INF, NINF):
        if a == 0 or b == 0:
            return NAN, 0
        p = NINF if p_neg else INF
        if acc in (INF, NINF) and acc != p:
            return NAN, 0
        return p, p_neg
    if acc in (INF, NINF):
        return acc, acc_neg
    p, scale = a * b, 2 * U
    if unfused and p != 0:
        p, scale = round_units(p, 2 * U), U
        if p in (INF, NINF):
            return p, p_neg
        if flush_out:
            p = _flush(p)
    n = p + (acc << (scale - U))
    if n == 0:
        # exact zero: -0 only when both terms are negative zeros (or a zero product / rounded product and -0)
        return 0, int(p == 0 and acc == 0 and p_neg and acc_neg)
    out = round_units(n, scale)
    if flush_out:
        out = _flush(out)
    return out, int(n < 0)


def exact_chain(qrow, rrow, metric=0, flush_in=False, flush_out=False, unfused=False, descending=False):
    """the chain of one pair of rows -> np.float32; the keyword faults are the deliberately wrong variants"""
    acc, acc_neg = 0, 0
    ks = range(len(qrow) - 1, -1, -1) if descending else range(len(qrow))
    for k in ks:
        if metric == 1:
            df = np.float32(qrow[k]) - np.float32(rrow[k])      # (only the L2 difference uses float arithmetic: one IEEE op)
            (a, an), (b, bn) = to_units(df), to_units(df)
        else:
            (a, an), (b, bn) = to_units(qrow[k]), to_units(rrow[k])
        if flush_in:
            a, b = _flush(a), _flush(b)
        acc, acc_neg = fma_step(a, an, b, bn, acc, acc_neg, unfused, flush_out)
    return to_f32(acc, bool(acc_neg))


def exact_scores(q, r, **kw):
    return np.array([[exact_chain(a, b, **kw) for b in r] for a in q], dtype=np.float32)


def isqrt_round(a):
    """sqrt(a 2^-149) correctly rounded to float32, in units of 2^-149 (a > 0)"""
    s = 30
    n = (2 * a) << (2 * s)                  # sqrt(a 2^-149) = sqrt(2a 2^2s) 2^(-s - 75)
    root = math.isqrt(n)
    n2 = 2 * root + (1 if root * root != n else 0)       # one sticky bit below the floor of the root
    return round_units(n2, s + 75 + 1)


def exact_divide(x, x_neg, nrm):
    """x / nrm rounded once (both in units of 2^-149, nrm > 0 finite or INF)"""
    if x == 0:
        return to_f32(0, bool(x_neg))
    if nrm == INF:
        return to_f32(0, bool(x_neg))
    s = 200
    num = abs(x) << s
    quo, rem = divmod(num, nrm)
    n2 = 2 * quo + (1 if rem else 0)
    out = round_units(-n2 if x < 0 else n2, s + 1)
    return to_f32(out, bool(x_neg))


def exact_normalize(x):
    out = np.empty_like(x)
    for i, row in enumerate(x):
        acc, neg = 0, 0
        for v in row:
            a, an = to_units(v)
            acc, neg = fma_step(a, an, a, an, acc, neg)
        nrm = INF if acc == INF else ((1 << U) if acc == 0 else isqrt_round(acc))     # a zero norm is replaced by 1
        for k, v in enumerate(row):
            a, an = to_units(v)
            out[i, k] = exact_divide(a, an, nrm)
    return out


def same(a, b):
    """bits equal; NaN positions compared as a set (payloads are not part of the contract)"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


# ---------------------------------------------------------------- the restatement itself
def test_restatement_on_known_values():
    f = np.float32
    tiny = f(2.0 ** -149)
    assert bits(exact_chain([f(2.0 ** -75)], [f(2.0 ** -75)]))[0] == 0            # 2^-150: tie, rounds to even = +0
    assert bits(exact_chain([f(-2.0 ** -75)], [f(2.0 ** -75)]))[0] == 0x80000000   # ... and to -0
    assert exact_chain([f(1.5 * 2.0 ** -75)], [f(2.0 ** -75)]) == tiny             # 1.5 x 2^-150 rounds up
    assert exact_chain([f(2.0 ** 64)] * 2, [f(2.0 ** 64), f(-2.0 ** 64)]) == np.inf  # overflowed, then stays
    assert np.isnan(exact_chain([f(-2.0 ** 64), f(1)], [f(2.0 ** 64), f(np.inf)]))  # -inf + inf
    a, b = f(1 + 2.0 ** -23), f(1 - 2.0 ** -23)
    assert exact_chain([f(1), a], [f(-1), b]) == f(-2.0 ** -46)                     # fused: the product's low bits survive
    assert exact_chain([f(1), a], [f(-1), b], unfused=True) == 0
    assert exact_chain([f(1), a], [f(-1), b], descending=True) == 0
    assert exact_chain([f(2.0 ** -130)], [f(2.0 ** 10)], flush_in=True) == 0
    assert exact_chain([f(2.0 ** -70)], [f(2.0 ** -60)], flush_out=True) == 0


# ---------------------------------------------------------------- 1. the oracle against the exact restatement
@pytest.mark.parametrize("d", cc.DIMS)
@pytest.mark.parametrize("name", cc.CLASSES)
def test_oracle_scores_equal_the_exact_chain(orc, name, d):
    q, r = cc.make(name, d, 7, 9, seed=1)
    ref = exact_scores(q, r)
    assert same(orc.scores(q, r), ref)
    for bias in (0.0, 0.5):
        with np.errstate(invalid="ignore", over="ignore"):
            # (`acc + bias` also with bias 0: a -0.0 similarity becomes +0.0, as in the oracle and in tn_sims.h)
            assert same(orc.pair_sims(q, r, bias), ref + np.float32(bias))
    if d <= 100:
        ql, rl = cc.make(name, d, 7, 9, seed=1, scale=0.5) if name == "overflow" else (q, r)
        with np.errstate(invalid="ignore", over="ignore"):
            assert same(orc.scores(ql, rl, 1), exact_scores(ql, rl, metric=1))


@pytest.mark.parametrize("d", [7, 64, 511])
def test_oracle_row_normalize_equals_the_exact_restatement(orc, d):
    x = cc.normalize_rows(13, d, seed=1)
    with np.errstate(all="ignore"):
        got = orc.row_normalize(x)
    assert same(got, exact_normalize(x))


# ---------------------------------------------------------------- 2. discriminating power
AIMED = [("sub_in", "flush_in"), ("sub_out", "flush_out"), ("cancel", "unfused"), ("cancel", "descending"),
         ("overflow", "descending"), ("overflow", "unfused"), ("mixed_tile", "flush_in"), ("mixed_tile", "flush_out")]
FLOOR = {("mixed_tile", "flush_in"): 0.1, ("mixed_tile", "flush_out"): 0.02}   # a sixth / a thirtieth of its pairs are of that class


# `overflow` is aimed at the order; it also shows fusion from d = 64 on (0.43 of the pairs).  At d = 3 half of its pairs are
# +-inf or NaN whatever the fusion, and the finite ones have two steps after the first (which is `fl(p0)` either way):
# 0.17 of the pairs differ there, so that combination is not asserted -- `cancel` carries fusion at d = 3 (0.5 and more).
FAULT_CASES = [(n, f, d) for n, f in AIMED for d in cc.DIMS if not ((n, f, d) == ("overflow", "unfused", 3))]


@pytest.mark.parametrize("name,fault,d", FAULT_CASES)
def test_each_fault_shows_on_the_class_aimed_at_it(orc, name, fault, d, capsys):
    q, r = cc.make(name, d, 12, 14, seed=2)
    ref = orc.scores(q, r)
    wrong = exact_scores(q, r, **{fault: True})
    nan = np.isnan(ref) | np.isnan(wrong)
    differ = (np.isnan(ref) != np.isnan(wrong)) | (~nan & (bits(ref) != bits(wrong)))
    share = float(differ.mean())
    with capsys.disabled():
        print(f"\n  chain fault {fault:10s} on {name:10s} d={d:3d}: {share:.3f} of the pairs differ", end="")
    assert share >= FLOOR.get((name, fault), 0.25), (name, fault, d, share)


# ---------------------------------------------------------------- 3. class shares
@pytest.mark.parametrize("d", cc.DIMS)
def test_class_shares(orc, d):
    q, r = cc.make("sub_in", d)
    assert (np.abs(r) < cc.SUBNORMAL).all() and (r != 0).all()
    s = orc.scores(q, r)
    assert (np.abs(s) >= cc.SUBNORMAL).all() and np.isfinite(s).all()

    q, r = cc.make("sub_out", d)
    s = orc.scores(q, r)
    assert (np.abs(s) < 2.0 ** -125).all() and np.mean(np.abs(s) < cc.SUBNORMAL) > 0.9 and np.mean(s != 0) > 0.9

    q, r = cc.make("underflow_zero", d)
    s = orc.scores(q, r)
    j = np.arange(cc.NR)
    assert (bits(s[:, j % 3 == 0]) == 0).all() and (bits(s[:, j % 3 == 1]) == 0x80000000).all()
    so = s[:, j % 3 == 2]
    assert (so != 0).all() and (so[1::3] < 0).all() and (so[2::3] > 0).all()
    assert 0.2 < np.mean(so[0::3] > 0) < 0.8

    q, r = cc.make("overflow", d)
    s = orc.scores(q, r)
    shares = [np.mean(s == np.inf), np.mean(s == -np.inf), np.mean(np.isnan(s)), np.mean(np.isfinite(s))]
    assert min(shares) >= 0.05 and shares[0] < 0.08, shares         # (+inf stays below the bulk K's tenth of the pairs)
    clean, hot = cc.finite_rows(r), np.arange(cc.NQ) % 3 == 2
    assert np.isfinite(s[~hot][:, clean]).all()                       # calm rows: finite against every unplanted reference
    blocks = clean & ((np.arange(cc.NR) // 3) % 5 == 2)
    exact = (q.astype(np.float64)[hot][:, None, :] * r.astype(np.float64)[None, blocks, :]).sum(axis=2)
    assert (np.abs(exact) < 2.0 ** 128).all() and np.isinf(s[hot][:, blocks]).all()    # exact sum finite, chain overflowed
    assert blocks.sum() * hot.sum() >= 0.03 * s.size
    qn, rn = cc.without_nan_rows(q, r)
    assert len(rn) == 200 and not np.isnan(orc.scores(qn, rn)).any()

    q, r = cc.make("cancel", d)
    s = orc.scores(q, r).astype(np.float64)
    big = np.abs(q.astype(np.float64)[:, None, :] * r.astype(np.float64)[None, :, :]).max(axis=2)
    assert np.isfinite(s).all() and np.median(np.abs(s) / big) < 2.0 ** -10      # the score is what cancellation left

    q, r = cc.make("mixed_tile", d)
    for x, period in ((q, 6), (r, 7)):
        norms = np.linalg.norm(x.astype(np.float64), axis=1)
        unitrow = np.abs(norms - 1.0) < 1e-3
        assert unitrow[period - 1::period].all()
        for t0 in range(0, len(x) - 31, 32):          # every 32-row block holds ordinary rows and rows of the classes
            assert unitrow[t0:t0 + 32].any() and (~unitrow[t0:t0 + 32]).sum() >= 16


# ---------------------------------------------------------------- 4. where the searches of the GPU file cut
@pytest.mark.parametrize("nr", [cc.NR, cc.NR_WIDE])
@pytest.mark.parametrize("d", cc.DIMS)
@pytest.mark.parametrize("name", cc.CLASSES)
def test_search_thresholds_cut_inside_the_score_range(orc, name, d, nr):
    q, r = cc.make(name, d, cc.NQ, nr)
    s = orc.scores(q, r)
    valid = s[~np.isnan(s)]
    lo, hi = valid.min(), valid.max()
    # the thresholded range search
    rad = cc.range_radius(name, s)
    assert lo < rad < hi
    n_hits = int(orc.range_search(q, r, rad)[0][-1])
    assert 0 < n_hits < valid.size
    # global top-K: the bulk and the small K re-threshold at least once and end on a radius inside the range
    for label, K in cc.topk_cases(name, s.size).items():
        oi, oj, os_, info = orc.global_threshold_search(q, r, K, 0, return_info=True)
        assert info["n_rethreshold"] >= 1, (label, K, info)
        if label == "inf":
            # the one K on the +inf tie: the cut falls on it and drops all of it (the comparison is strict)
            assert info["radius"] == np.inf and len(os_) == 0, (label, info)
            continue
        assert lo < info["radius"] < hi and np.isfinite(info["radius"]) and len(os_) > 0, (label, K, info, lo, hi)
        if label == "zero":
            assert info["radius"] == 0 and len(os_) < K           # every hit tied with the zero radius is dropped
    if name == "underflow_zero":
        # a K whose cut falls on the zeros without a re-threshold at that value: +0.0 and -0.0 tie, reference order decides
        K = s.size // 2
        oi, oj, os_, info = orc.global_threshold_search(q, r, K, 0, return_info=True)
        tail = bits(os_[-200:])
        assert len(os_) == K and (os_[-200:] == 0).all() and (tail == 0).any() and (tail == 0x80000000).any()
    # k-NN on the rows without NaN scores: the k-th score of at least a third of the rows lies strictly inside the range
    qn, rn = cc.without_nan_rows(q, r)
    for k in cc.KNN_KS:
        D, _ = orc.knn(qn, rn, k)
        inside = (D[:, k - 1] > lo) & (D[:, k - 1] < hi)
        assert inside.mean() >= 1 / 3, (k, inside.mean())
        if name == "underflow_zero":
            assert (D[1::3, k - 1] == 0).all()             # rows i % 3 == 1: every k-th score is a zero


def test_oracle_knn_leaves_slots_empty_for_scores_below_the_heap_sentinel(orc):
    """faiss fills its result heap with -FLT_MAX / +FLT_MAX and id -1 and inserts on a strict comparison: -inf (inner
    product), +inf (L2) and NaN never enter, whatever k."""
    big = np.float32(2.0 ** 100)
    q = np.array([[1, 0], [1, 1], [big, big]], np.float32)
    r = np.array([[1, 0], [-big, -big], [2, 0], [np.inf, -np.inf], [-big, 0]], np.float32)
    s = orc.scores(q, r)
    assert np.array_equal(s[2, [1, 4]], [-np.inf, -np.inf]) and np.isnan(s[:, 3]).all()
    D, I = orc.knn(q, r, 4)
    fmax = np.finfo(np.float32).max
    assert I.tolist() == [[2, 0, 1, 4], [2, 0, 4, 1], [2, 0, -1, -1]]       # (row 0: the references 1 and 4 tie)
    assert np.array_equal(D[2], np.array([2 * big, big, -fmax, -fmax], np.float32))
    D, I = orc.knn(q, r, 2, 1)      # L2: (1 + big)^2 is finite, (big + big)^2 overflows; row 2 is 2^100 away from all
    assert I[:2].tolist() == [[0, 2], [0, 2]] and I[2].tolist() == [-1, -1]
    D, I = orc.knn(q[2:], r[[1, 3, 4]], 2, 1)
    assert I.tolist() == [[-1, -1]] and np.array_equal(D[0], np.array([fmax, fmax], np.float32))
