"""Input classes that take the fp32 chain `acc = fmaf(q[k], r[k], acc)` (k ascending, from +0)
out of the normal range: subnormal operands, subnormal sums, products that underflow to +-0, chains that overflow
half-way, cancellations that leave only rounding residue, and all of them mixed with ordinary rows in every tile.

Plain numpy, seeded.  `make(name, d)` returns (q, r) as float32; tests/test_chain_contract_host.py asserts on the CPU
that every class is what it claims to be, tests/test_gpu_chain_contract.py runs the classes through every device
implementation of the chain.

Sizes: NQ = 130 crosses the 128-row query tile and the 64-row wave tile, NR = 300 (NR_WIDE = 1500 where a pre-filter
route needs several 512-column steps); d = 3 (below one k-group), 64 (exact), 100 (no multiple of 8), 512.

A chain of FINITE operands never yields NaN: the product inside fmaf is not rounded, so it is never infinite, and
`inf + finite` stays inf.  `overflow` therefore plants one +inf element at the end of a third of its reference rows:
where the chain has already overflowed the other way, that last step is `inf - inf`.
"""
import numpy as np

NQ, NR, NR_WIDE = 130, 300, 1500
DIMS = (3, 64, 100, 512)
CLASSES = ("sub_in", "sub_out", "underflow_zero", "overflow", "cancel", "mixed_tile")
SUBNORMAL = np.float32(2.0 ** -126)      # |x| < SUBNORMAL: subnormal or zero


def _mag(rng, shape, lo=1.0, hi=2.0):
    return rng.uniform(lo, hi, shape)


def _signs(rng, shape):
    return rng.choice(np.array([-1.0, 1.0]), size=shape)


def _f32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32)


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d))
    return _f32(x / np.linalg.norm(x, axis=1, keepdims=True))


def sub_in(d, nq, nr, rng, q_exp=100):
    """r: every element an fp32 subnormal (2^-148 <= |x| < 2^-126); q ~ 2^100 N(0, 1): products ~2^-37, all normal."""
    r = _signs(rng, (nr, d)) * _mag(rng, (nr, d)) * 2.0 ** rng.integers(-148, -126, (nr, d))
    q = rng.standard_normal((nq, d)) * 2.0 ** q_exp
    return _f32(q), _f32(r)


def sub_out(d, nq, nr, rng):
    """|q[k]|, |r[k]| in [2^-71, 2^-67): products in [2^-142, 2^-134), every partial sum below 2^-125 and nearly all
    of them subnormal; no product is a multiple of 2^-149, so every step rounds on the subnormal grid."""
    q = _signs(rng, (nq, d)) * _mag(rng, (nq, d)) * 2.0 ** rng.integers(-71, -68, (nq, d))
    r = _signs(rng, (nr, d)) * _mag(rng, (nr, d)) * 2.0 ** rng.integers(-71, -68, (nr, d))
    return _f32(q), _f32(r)


def underflow_zero(d, nq, nr, rng, q_exp=-41, tiny_exp=-115):
    """q: |q[k]| in [2^-41, 2^-40), last element positive.  References j % 3 == 0 / 1: |r[k]| in [2^-115, 2^-114), last
    element positive / negative: every product lies below 2^-153 and rounds to a zero with its own sign, so the score is
    +0.0 / -0.0 (the sign of the last product).  References j % 3 == 2: ordinary rows (unit Gaussian with a first coordinate
    of 8 .. 16), scores ~2^-36 of both signs.  Query rows i % 3 == 1 have q[0] < 0: all their ordinary scores are
    negative, so every k-th best score of those rows is a zero; rows i % 3 == 2 have q[0] > 0 (k-th score in the bulk),
    rows i % 3 == 0 a q[0] of random sign.  A global K of half the pairs falls on the zeros."""
    q = _signs(rng, (nq, d)) * _mag(rng, (nq, d)) * 2.0 ** q_exp
    q[:, d - 1] = np.abs(q[:, d - 1])
    i = np.arange(nq)
    q[i % 3 == 1, 0] = -np.abs(q[i % 3 == 1, 0]) * 4.0
    q[i % 3 == 2, 0] = np.abs(q[i % 3 == 2, 0]) * 4.0
    r = _signs(rng, (nr, d)) * _mag(rng, (nr, d)) * 2.0 ** tiny_exp
    j = np.arange(nr)
    r[j % 3 == 0, d - 1] = np.abs(r[j % 3 == 0, d - 1])
    r[j % 3 == 1, d - 1] = -np.abs(r[j % 3 == 1, d - 1])
    o = j % 3 == 2
    g = rng.standard_normal((int(o.sum()), d)) / np.sqrt(d)
    g[:, 0] = _mag(rng, len(g)) * 8.0      # (q[0] r[0] is 30 sigma of the other coordinates' sum: it decides the sign)
    r[o] = g
    return _f32(q), _f32(r)


def _sign_pattern(kind, d):
    k = np.arange(d)
    if kind == 0:                                   # C: constant
        return np.ones(d)
    if kind == 1:                                   # B: blocks of two, ++--++--
        return np.where((k // 2) % 2 == 0, 1.0, -1.0)
    return np.where(k % 2 == 0, 1.0, -1.0)          # A: alternating


def overflow(d, nq, nr, rng, scale=1.0, plant=3):
    """Full-size elements |x| in [1.42, 1.5) 2^63: one product (2.02-2.25 x 2^126) is finite, two of one sign in a row
    overflow.  Query rows i % 3 == 2 are HOT: full size, one sign s_i.  The other two thirds are CALM: random signs at
    2^-8 of that size (no run of their products comes near 2^128), last element negative: all their chains are finite.
    Reference rows are full size, by (j // 3) % 5: constant + / constant - / blocks of two (++--) / alternating /
    alternating.  A hot row overflows to +-inf at k = 1 against the constant rows, and against the blocks, where the
    next block would cancel the sum exactly and the descending order ends at the opposite infinity; against the alternating rows
    it stays finite (at d = 512 a few of those sums drift past 2^128 too).  References j % plant == 0 are constant - and end in +inf: a hot row sits at the opposite infinity by then
    or meets it in the last step: inf - inf = NaN; a calm row goes to -inf in that step.  Shares: +inf 1/15, -inf ~0.29,
    NaN 1/9, finite ~0.53; every score of a calm row outside the planted references is finite (k-th scores, bulk cuts).
    scale = 0.5 (L2): `(q - r)^2` of two full-size elements of opposite sign is 2.1 x 2^126, the second one overflows."""
    i, j = np.arange(nq), np.arange(nr)
    hot = i % 3 == 2
    q = _signs(rng, (nq, d)) * _mag(rng, (nq, d), 1.42, 1.5) * 2.0 ** 55 * scale
    q[:, d - 1] = -np.abs(q[:, d - 1])
    q[hot] = _mag(rng, (int(hot.sum()), d), 1.42, 1.5) * 2.0 ** 63 * scale * np.where((i[hot] // 3) % 2 == 0, 1.0, -1.0)[:, None]
    kind = (j // 3) % 5
    pattern = np.stack([_sign_pattern(0, d), -_sign_pattern(0, d), _sign_pattern(1, d), _sign_pattern(2, d), -_sign_pattern(2, d)])
    r = _mag(rng, (nr, d), 1.42, 1.5) * 2.0 ** 63 * scale * pattern[kind]
    planted = j % plant == 0
    r[planted] = -np.abs(r[planted])
    q, r = _f32(q), _f32(r)
    r[planted, d - 1] = np.inf
    return q, r


def cancel(d, nq, nr, rng, span=20):
    """Exponents spread over +-`span` binades per operand (+-40 for the products).  Coordinates come in couples (2t, 2t + 1)
    with q[2t+1] = q[2t] c_t and r[2t+1] = -r[2t] / c_t, each rounded to fp32: for EVERY pair of rows the second product
    cancels the first up to ~2^-23 of it, and what remains of a step is the rounding residue of the steps before it.  The
    score depends on whether the product is rounded before the addition, and on the order of the steps."""
    def base(n):
        return _signs(rng, (n, d)) * _mag(rng, (n, d)) * 2.0 ** rng.integers(-span, span + 1, (n, d))

    q, r = _f32(base(nq)).astype(np.float64), _f32(base(nr)).astype(np.float64)
    c = _mag(rng, d // 2) * 2.0 ** rng.integers(-3, 4, d // 2)
    for t in range(d // 2):
        q[:, 2 * t + 1] = q[:, 2 * t] * c[t]
        r[:, 2 * t + 1] = -r[:, 2 * t] / c[t]
    if d % 2:    # (the coordinate without a partner is the smallest, or its product would be the score)
        q[:, d - 1] = _signs(rng, nq) * _mag(rng, nq) * 2.0 ** -span
        r[:, d - 1] = _signs(rng, nr) * _mag(rng, nr) * 2.0 ** -span
    return _f32(q), _f32(r)


_BUILDERS = dict(sub_in=sub_in, sub_out=sub_out, underflow_zero=underflow_zero, overflow=overflow, cancel=cancel)


def mixed_tile(d, nq, nr, rng):
    """The first rows of the five classes above and unit Gaussian rows interleaved: query rows with period 6, reference
    rows with period 7 (two Gaussian rows), so every class meets every class, and every 32 x 32 MFMA block and every
    128-row int8 panel holds both kinds.  Here `sub_in`'s queries are at 2^50 (at 2^100 their products with `overflow`'s
    references would all be infinite) and `overflow` plants +inf in every ninth of its references: +inf scores stay near
    1 % of the pairs, below the smallest K of the searches."""
    kw = dict(sub_in=dict(q_exp=50), overflow=dict(plant=9))
    parts = [b(d, nq, nr, rng, **kw.get(n, {})) for n, b in _BUILDERS.items()]
    q, r = unit_rows(rng, nq, d), unit_rows(rng, nr, d)
    for t in range(5):
        q[t::6] = parts[t][0][:len(q[t::6])]
        r[t::7] = parts[t][1][:len(r[t::7])]
    return q, r


def make(name, d, nq=NQ, nr=NR, seed=0, **kw):
    """(q [nq, d], r [nr, d]) float32 of class `name`; the same arguments give the same rows."""
    rng = np.random.default_rng([seed, CLASSES.index(name), d])
    if name == "mixed_tile":
        return mixed_tile(d, nq, nr, rng)
    return _BUILDERS[name](d, nq, nr, rng, **kw)


def finite_rows(x):
    """mask of the rows without inf / NaN elements (the others are the NaN-producing rows of `overflow`)"""
    return np.isfinite(x).all(axis=1)


def without_nan_rows(q, r):
    return np.ascontiguousarray(q[finite_rows(q)]), np.ascontiguousarray(r[finite_rows(r)])


# ---- the searches every route runs on a class (the GPU file runs them, the host file asserts where they cut)
KNN_KS = (1, 7, 33)


def topk_cases(name, n_pairs):
    """{label: K} of the global top-K searches, all with re-threshold events (2K below the number of kept hits): a small K
    (a fiftieth of the pairs), a K in the bulk (a tenth), and the K that puts the cut on the class's special values: on
    the zeros of `underflow_zero` (positive scores are a sixth of the pairs, zeros two thirds).  `overflow`'s +inf scores
    are a fifteenth of the pairs: its small K is the K on the inf tie, its bulk K and a wider one (an eighth; a third of the pairs is finite and
    positive) cut among the finite scores."""
    ks = {"small": n_pairs // 50, "bulk": n_pairs // 10}
    if name == "underflow_zero":
        ks["zero"] = n_pairs // 4
    if name == "overflow":
        ks = {"inf": ks["small"], "bulk": ks["bulk"], "wide": n_pairs // 8}
    return ks


def range_radius(name, scores, metric=0):
    """The radius of the thresholded range search: 0.0 for `underflow_zero` (on the zeros: neither +0.0 nor -0.0 is a
    hit), else the score that a tenth of the finite scores lie beyond (an actual score: the comparison is strict)."""
    if name == "underflow_zero" and metric == 0:
        return np.float32(0.0)
    s = np.sort(scores[np.isfinite(scores)].ravel())
    if len(s) == 0:      # (`sub_in` under L2: every distance is +inf)
        return np.float32(1.0)
    return s[len(s) // 10] if metric == 1 else s[len(s) - 1 - len(s) // 10]


# ---- variants that half floats can hold (SQfp16 stores the references rounded to fp16)
def fp16_cases(d, nq=NQ, nr=NR, seed=0):
    """{name: (q, r)}: `cancel` with the exponents inside fp16's normal range, `mixed_tile` of it with Gaussian rows,
    and `underflow_zero` with reference rows that are SUBNORMAL in fp16 (|r[k]| in [2^-22, 2^-21); q at 2^-133 .. 2^-130 is
    subnormal in fp32, the products lie below 2^-150)."""
    rng = np.random.default_rng([seed, 99, d])
    cq, cr = cancel(d, nq, nr, rng, span=5)
    mq, mr = unit_rows(rng, nq, d), unit_rows(rng, nr, d)
    mq[::2], mr[::3] = cq[::2], cr[::3]
    uq, ur = underflow_zero(d, nq, nr, rng, q_exp=-133, tiny_exp=-22)
    return {"cancel": (cq, cr), "mixed_tile": (mq, mr), "underflow_zero": (uq, ur)}


# ---- rows for vsc_row_normalize
def normalize_rows(n, d, seed=0):
    """Rows cycling through: sub_out-like elements (x^2 subnormal), elements ~2^-80 (sum x^2 underflows to 0 while x != 0),
    elements ~2^70 (sum x^2 overflows), a zero row, a unit Gaussian row, subnormal elements."""
    rng = np.random.default_rng([seed, 77, n, d])
    x = np.empty((n, d))
    for i in range(n):
        s, m = _signs(rng, d), _mag(rng, d)
        t = i % 6
        if t == 0:
            x[i] = s * m * 2.0 ** rng.integers(-71, -68, d)
        elif t == 1:
            x[i] = s * m * 2.0 ** -80
        elif t == 2:
            x[i] = s * m * 2.0 ** 70
        elif t == 3:
            x[i] = 0.0
        elif t == 4:
            x[i] = rng.standard_normal(d)
        else:
            x[i] = s * m * 2.0 ** rng.integers(-148, -127, d)
    if n == 1:
        x[0] = _signs(rng, d) * _mag(rng, d) * 2.0 ** -80
    return _f32(x)
