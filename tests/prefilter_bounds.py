"""Inputs that bring the fp16 and int8 pre-filters' error bounds within a few per cent of the real error, and a float64
restatement of what the kernels compute for them (test_prefilter_bounds.py on the CPU, test_gpu_prefilter_bounds.py
on the device).

Random or descriptor-like rows never get there: their rounding errors cancel in the dot product and stay far below the
bounds.  Here every rounding error of a planted pair points the same way:

* int8 (quant_i8.hip): one coordinate of every row is +-127 2^k, so the scale amax / 127 is exactly 2^k; every other
  coordinate is +-(M + 63/128) 2^k, so each residual is 63/128 of a step with the sign of its coordinate.  A query and
  its planted partner share one sign pattern: e_x . q_y and q_x . e_y add up, and s_x s_y (q_x . q_y) lies below x . y
  by ~0.98 of E_x N'_y + (N'_x + E_x) E_y.  All rows have the same magnitude profile, so a 128-row query panel (one
  scale, the largest E and N of its rows) is as tight as a single row.
* fp16 (layout.hip): every coordinate is +-(1 + 2^-11 - 2^-22) 2^e, just below the midpoint between two fp16 values;
  all of them round down by ~2^-11 relative, the pair's products by ~2^-10: the whole (2^-10 + 2^-22) share of c1.

Every value sits on a power-of-two grid, so the scales, residuals, centred rows and means are exact, and all planted
pairs have one fp32 chain score (the same products in the same order).

Decoys set the threshold just below that score: a reference equal to the query's partner but one step smaller in its
last coordinate (score s_d < s by ~0.1-2 % of the bound).  `topk_case` puts K + 1 decoys into the first batch of the
global top-K schedule (its radius becomes s_d), `knn_case` puts a decoy (and k - 1 references that score above the
partner) in front of the partner in reference order (the k-NN's threshold when it reaches the partner's range is s_d).
"""
import math

import numpy as np

FRAC = 63.0 / 128.0      # int8: residual of every non-extreme coordinate, in steps of the scale
M = 100.0                # int8: integer part of those coordinates
F16_MID = 1.0 + 2.0 ** -11 - 2.0 ** -22     # fp16: just below the midpoint between 1 and 1 + 2^-10
F16_MID_UP = 1.0 + 2.0 ** -11 + 2.0 ** -22  # fp16: just above it (defer_radius_case: every coordinate rounds up)

# fraction of c1 |q||r| that the fp16 construction reaches, asserted per dimension (D = 1000 pads to 1024)
F16_REACH = {64: 0.95, 512: 0.85, 768: 0.75, 1000: 0.75}
I8_REACH = 0.97
I8_MARGIN = 0.9          # int8: low + 0.9 eps < threshold: a bound 10 % tighter loses every planted pair


def _round_up(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------- the rows
class Case:
    """q, r (float32 rows), partner[i] = the planted reference of query row i (-1: none); `exclude` = (coordinate,
    value every reference holds there), `mu` = the references' exact mean (centred case)"""

    def __init__(self, q, r, partner, kind, d, exclude=None, mu=None):
        self.q, self.r, self.partner = q, r, partner
        self.kind, self.d, self.exclude, self.mu = kind, d, exclude, mu

    def planted(self):
        rows = np.flatnonzero(self.partner >= 0)
        return rows, self.partner[rows]


def row_exponent(kind, d):
    """power-of-two row factor that brings the rows to norm ~1"""
    base = (M + FRAC) if kind == "i8" else 1.0
    return -int(round(math.log2(base * math.sqrt(d))))


def magnitudes(kind, d, level=0, mid=F16_MID):
    """|coordinates| of a row.  level 0: queries, partners, noise; -1: decoy (last coordinate one int8 step / 2^-11
    smaller: the score drops below the partner's in the chain's last addition); +1 (k-NN): one step larger.
    mid (fp16): F16_MID, all coordinates round down (low < exact), or F16_MID_UP, all round up (low > exact)"""
    k = row_exponent(kind, d)
    if kind == "i8":
        a = np.full(d, (M + FRAC) * 2.0 ** k)
        a[0] = 127.0 * 2.0 ** k
        a[d - 1] += level * 2.0 ** k
    else:
        a = np.full(d, mid * 2.0 ** k)
        a[d - 1] += level * 2.0 ** (k - 11)
    return a


def _signs(rng, n, d, fixed=0):
    s = rng.choice(np.array([-1.0, 1.0]), size=(n, d))
    s[:, :fixed] = 1.0                    # (centred case: x . mu is the same for every query row)
    return s


def _assemble(kind, d, nq, nr, roles, rng, exclude=False, centre=False):
    """roles: per query row a list of (level, count, where) -- where = 'early' (first quarter of the references) or
    'late' (last quarter; level 0 = the partner).  Noise rows (random signs, same magnitudes) fill the middle."""
    fixed = 8 if centre else 0
    sq = _signs(rng, nq, d, fixed)
    q = sq * magnitudes(kind, d, 0)
    early, late, partner_rel = [], [], np.full(nq, -1, np.int64)
    for i, rl in enumerate(roles):
        for level, count, where in rl:
            row = sq[i] * magnitudes(kind, d, level)
            if where == "late":
                partner_rel[i] = len(late)
                late.append(row)
            else:
                early.extend([row] * count)
    early = np.array(early).reshape(-1, d)
    late = np.array(late).reshape(-1, d)
    assert len(early) <= nr // 4 - 64 and len(late) <= nr // 4 - 64, (len(early), len(late), nr)
    if centre:
        # references = mu + pattern, patterns in +- pairs: the mean of the references is exactly mu
        n_noise = nr - 2 * (len(early) + len(late))
        assert n_noise >= 0 and n_noise % 2 == 0
        noise = _signs(rng, n_noise // 2, d) * magnitudes(kind, d, 0)
        middle = np.concatenate([-early, -late, noise, -noise])
    else:
        middle = _signs(rng, nr - len(early) - len(late), d) * magnitudes(kind, d, 0)
    r = np.concatenate([early, middle, late])
    partner = np.where(partner_rel >= 0, len(r) - len(late) + partner_rel, -1)
    ex = mu = None
    if exclude:
        # one coordinate equal on every reference, four times the largest one: the image leaves it out and it acts
        # through the rows' thresholds (the same value in every query row keeps all planted scores equal)
        c = d // 2
        v = 4.0 * 127.0 * 2.0 ** row_exponent(kind, d)
        r[:, c] = v
        q[:, c] = (M + FRAC) * 2.0 ** row_exponent(kind, d)
        ex = (c, v)
    if centre:
        mu = np.zeros(d)
        mu[:fixed] = 32.0 * 2.0 ** row_exponent(kind, d)
        r = r + mu
    q32, r32 = q.astype(np.float32), r.astype(np.float32)
    assert np.array_equal(q32.astype(np.float64), q) and np.array_equal(r32.astype(np.float64), r)  # all exact
    return Case(q32, r32, partner, kind, d, ex, mu)


def decoys(c, rows):
    """the decoy of each query row in `rows`: its partner with the last coordinate one step smaller"""
    dec = np.sign(c.q[rows].astype(np.float64)) * magnitudes(c.kind, c.d, -1)
    if c.exclude is not None:
        dec[:, c.exclude[0]] = c.exclude[1]
    if c.mu is not None:
        dec = dec + c.mu
    return dec.astype(np.float32)


def topk_case(kind, d, nq=480, nr=8192, seed=0, **kw):
    """Global top-K: the first batch (32 rows) holds 15 decoys per row and no partner, every later row one partner.
    K = the number of partners: after the first batch the radius is the (K+1)-th best score = s_d, and every planted
    pair of the later batches meets the pre-filter at that radius."""
    rng = np.random.default_rng(seed)
    roles = [[(-1, 15, "early")] if i < 32 else [(0, 1, "late")] for i in range(nq)]
    c = _assemble(kind, d, nq, nr, roles, rng, **kw)
    c.K = nq - 32
    assert 32 * 15 >= c.K + 1
    return c


def knn_case(kind, d, k, nq=256, nr=8192, seed=1, **kw):
    """k-NN: per query row k - 1 references above the partner and one decoy in the first quarter of the references,
    the partner in the last quarter.  The forced k-NN (api_knn.hip) visits the references past its exact first pass in
    ranges that grow 3x, and its last range starts between a quarter and three quarters of them: the partner's range is
    searched with the row's threshold at s_d, and the partner is rank k."""
    rng = np.random.default_rng(seed)
    roles = [[(1, k - 1, "early"), (-1, 1, "early"), (0, 1, "late")] for _ in range(nq)]
    return _assemble(kind, d, nq, nr, roles, rng, **kw)


# ---------------------------------------------------------------- float64 restatement of the kernels
def _norm_up(ss, n):
    """quant_i8.hip norm_up"""
    return np.sqrt(ss) * 1.001 + 2.2e-19 * math.sqrt(n)


def i8_quantise(x, exclude=None, mu=None, panel=False):
    """quant_ref_frag_kernel (panel=False: one scale per row) / quant_query_panels_kernel (panel=True: one scale for
    all rows given).  Returns (scale, q, E, N, N') -- per row, or the panel's one scale and largest E, N, N'."""
    x = np.asarray(x, np.float64)
    d = x.shape[1]
    dpad = _round_up(d, 64)
    v = x.copy()
    if mu is not None:
        v = (x.astype(np.float32) - np.asarray(mu, np.float32)).astype(np.float64)
    if exclude is not None:
        v[:, exclude[0]] = 0.0
    amax = np.abs(v).max(axis=1)
    if panel:
        amax = np.full(len(v), amax.max())
    s = (amax.astype(np.float32) / np.float32(127.0)).astype(np.float64)
    inv = (np.float32(1.0) / s.astype(np.float32)).astype(np.float64)
    qi = np.clip(np.rint((v * inv[:, None]).astype(np.float32)), -127, 127).astype(np.float64)
    res = v - s[:, None] * qi
    E = _norm_up((res * res).sum(1), dpad)
    N = _norm_up((x * x).sum(1), dpad)
    Nk = _norm_up((v * v).sum(1), dpad)
    if mu is not None:
        E = E + 6.0e-8 * Nk
    if panel:
        return s[0], qi, E.max(), N.max(), Nk.max()
    return s, qi, E, N, Nk


def i8_eps(Eq, Nq, Nkq, Er, Nr, Nkr, d):
    """sim_i8p.hip: eps = (E_q N'_r + (N'_q + E_q) E_r + c_acc N_q N_r) x 1.001, c_acc = (dpad + 2) 2^-23"""
    c_acc = (_round_up(d, 64) + 2.0) * 2.0 ** -23
    return (Eq * Nkr + (Nkq + Eq) * Er + c_acc * Nq * Nr) * 1.001


def f16_coefficients(d):
    """api_search.hip: c1, c2, c3 for the padded dimension"""
    D = float(_round_up(d, 128))
    c1 = 2.0 ** -10 + 2.0 ** -22 + (2.0 * D + D / 16.0 + 16.0) * 2.0 ** -23
    c2 = 2.0 ** -25 * 1.001 * math.sqrt(D)
    c3 = D * 2.0 ** -50
    return c1, c2, c3


def f16_eps(nq, nr, d):
    c1, c2, c3 = f16_coefficients(d)
    return (c1 * nq * nr + c2 * (nq + nr) + c3) * 1.001


def chain(x, y):
    """the fp32 ascending-k fma chain of every row pair (x[n], y[n]) (the exact stage / the oracle)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    acc = np.zeros(len(x), np.float32)
    for kk in range(x.shape[1]):
        acc = (x[:, kk] * y[:, kk] + acc.astype(np.float64)).astype(np.float32)
    return acc


class PairBound:
    """What the kernels compute for the planted pairs (rows[n], refs[n]) of a Case, in float64:
      low    the low-precision score the kernel compares (int8: s_q s_r (q_x . q_y) over the coordinates the images hold;
             fp16: h(x) . h(y))
      shift  what the row's threshold loses before that comparison: the excluded coordinate's b = x_c v_c and the
             centre's x . mu (row_bias_thresholds, row_center)
      err    exact score - shift - low: the error the bound has to cover
      eps    the bound as the kernel builds it (norms, E, N, N' with their safety factors)"""

    def __init__(self, case, rows, refs):
        x = case.q[rows].astype(np.float64)
        y = case.r[refs].astype(np.float64)
        self.d = d = case.d
        self.exact = (x * y).sum(1)
        self.b = np.zeros(len(rows))
        self.c = np.zeros(len(rows))
        self.cmag = np.zeros(len(rows))
        if case.kind == "i8":
            ex, mu = case.exclude, case.mu
            # the query panel: 128 rows of one magnitude profile (any 128 rows of the case give its scale, E, N, N')
            panel = case.q[:128]
            sq, _, Eq, Nq, Nkq = i8_quantise(panel, ex, None, panel=True)
            sr, qr, Er, Nr, Nkr = i8_quantise(y, ex, mu)
            _, qx, _, _, _ = i8_quantise(np.concatenate([panel, x]), ex, None, panel=True)
            self.low = sq * sr * (qx[len(panel):] * qr).sum(1)
            if ex is not None:
                self.b = x[:, ex[0]] * ex[1]
            if mu is not None:
                m = np.asarray(mu, np.float64)
                self.c, self.cmag = x @ m, np.abs(x) @ np.abs(m)
            self.eps = i8_eps(Eq, Nq, Nkq, Er, Nr, Nkr, d)
            self.unit = sq * sr          # one step of the integer accumulator
            self.c1qr = None
        else:
            hx, hy = x.astype(np.float16).astype(np.float64), y.astype(np.float16).astype(np.float64)
            self.low = (hx * hy).sum(1)
            nx, ny = np.linalg.norm(x, axis=1), np.linalg.norm(y, axis=1)
            self.eps = f16_eps(np.linalg.norm(case.q.astype(np.float64), axis=1).max() * 1.0005, ny * 1.0005, d)
            # (the fp16 screen of rescore.hip builds its bound from the pair's own query row, not the panel's largest)
            self.eps_pair = f16_eps(nx * 1.0005, ny * 1.0005, d)
            self.c1qr = f16_coefficients(d)[0] * nx * ny
            self.unit = None
        self.shift = self.b + self.c
        self.err = self.exact - self.shift - self.low

    def reach(self):
        """err / eps, and for fp16 err / (c1 |q||r|): the share of the bound that the rounding errors really use
        (negative where the low-precision score lies above the exact one: the F16_MID_UP rows)"""
        return self.err / self.eps, (None if self.c1qr is None else self.err / self.c1qr)

    def slack(self, t):
        """what the kernels take off a threshold t on top of eps (all of it in the pair's favour): candidate_edge's
        2.4e-7 (|t| + eps); int8: quotient_low's 2e-6 relative + 1e-3, the floor and the non-strict test's -1 (two
        steps of the accumulator), row_bias_thresholds' 1.2e-7 (n mag + (dpad + 2) cmag + |t| + |b| + 2 |c|)"""
        t = np.abs(np.asarray(t, np.float64))
        s = 2.4e-7 * (t + self.eps)
        if self.unit is not None:
            s = s + 2e-6 * t + (1e-3 + 2.0) * self.unit
            s = s + 1.2e-7 * (2.0 * np.abs(self.b) + (_round_up(self.d, 64) + 2.0) * self.cmag + t + 2.0 * np.abs(self.c))
        return s

    def margin(self, t):
        """(t - shift - slack - low) / eps against the exact threshold t of the whole score: the kernel keeps the pair
        iff this is below 1 (up to its slack), and a bound f eps would lose it iff it is above f"""
        return (np.asarray(t, np.float64) - self.shift - self.slack(t) - self.low) / self.eps


# ---------------------------------------------------------------- deferred rescoring: the band (radius, floor]
# A pre-filtered batch of the global top-K leaves the exact score of a candidate uncomputed when its fp16 score proves
# that score to lie in (radius, floor] (api_search.hip "the deferred set"): low > radius + e and low <= floor - e.  The
# two cases below bring planted pairs within (f, 1) e of one of those edges, on the side where a too small e is wrong:
#   defer_floor_case   rows that round down (low < exact): exact = s > floor = s_d, low ~0.9 eps below s.  A narrower
#                      e puts them into D; the next event is still decided without D and drops them from the result.
#   defer_radius_case  rows that round up (low > exact): exact = s <= radius = s_u, low ~0.9 eps above s.  A narrower
#                      e puts them into D; D is re-scored at the end and the search reports pairs at or below the radius.
# "Plain" references sign(q_i) c 2^k (exact in fp16) score ~c s, hundreds of eps away from every edge: those with
# radius < c s <= floor are the pairs a correct band defers, the others set radius and floor.
DEFER_NQ, DEFER_K, DEFER_NR = 224, 300, 2048 + 37    # schedule 32 + 64 + 128 rows; the last column tile holds 37


class DeferCase(Case):
    """roles[name] = (query rows, references) of the pairs of one role; K, side ('floor' / 'radius')"""

    def __init__(self, q, r, partner, d, side, roles):
        super().__init__(q, r, partner, "f16", d)
        self.side, self.roles, self.K = side, roles, DEFER_K

    def pairs(self, *names):
        rows = np.concatenate([self.roles[n][0] for n in names])
        refs = np.concatenate([self.roles[n][1] for n in names])
        return rows, refs


def _defer_assemble(d, side, mid, entries_of, nr, seed):
    """entries_of(i) = [(role, level or None, plain factor or None), ...] of query row i.  The references of every
    fourth later row go behind the noise, their planted partners last: the last, partial 64-column tile holds planted
    pairs of the 64-row batch (a partial panel) and of the 128-row batch; the other partners lie in interior tiles."""
    rng = np.random.default_rng(seed)
    nq, k = DEFER_NQ, row_exponent("f16", d)
    sq = _signs(rng, nq, d)
    q = sq * magnitudes("f16", d, 0, mid)
    front, tail_other, tail_planted = [], [], []
    for i in range(nq):
        for role, level, c in entries_of(i):
            vec = sq[i] * (magnitudes("f16", d, level, mid) if c is None else np.full(d, c * 2.0 ** k))
            late = i >= 32 and i % 4 == 3
            (tail_planted if late and role == "planted" else tail_other if late else front).append((role, i, vec))
    n_noise = nr - len(front) - len(tail_other) - len(tail_planted)
    assert n_noise >= 512 and len(tail_planted) >= nr % 64 > 0, (n_noise, len(tail_planted), nr)
    noise = _signs(rng, n_noise, d) * magnitudes("f16", d, 0, mid)
    tail = tail_other + tail_planted
    r = np.concatenate([np.array([v for _, _, v in front]), noise, np.array([v for _, _, v in tail])])
    where = [(role, i, n) for n, (role, i, _) in enumerate(front)]
    where += [(role, i, len(front) + n_noise + n) for n, (role, i, _) in enumerate(tail)]
    roles = {}
    for role in sorted({w[0] for w in where}):
        roles[role] = (np.array([i for ro, i, _ in where if ro == role]), np.array([j for ro, _, j in where if ro == role]))
    partner = np.full(nq, -1, np.int64)
    partner[roles["planted"][0]] = roles["planted"][1]
    q32, r32 = q.astype(np.float32), r.astype(np.float32)
    assert np.array_equal(q32.astype(np.float64), q) and np.array_equal(r32.astype(np.float64), r)  # all exact
    return DeferCase(q32, r32, partner, d, side, roles)


def defer_floor_case(d, nr=DEFER_NR, seed=2):
    """Rows 0..31: 9 decoys (s_d) and one plain 0.75 row each: the event at row 32 sets the radius to the 0.75 score, the
    288 decoys stay, every rank gives floor = s_d.  Rows 32..223: the partner (s > s_d, not provably <= floor), one more
    decoy (s_d = floor: not provably either), a plain 0.875 row (deferred) and on every third row a plain 1.25 row."""
    def entries(i):
        if i < 32:
            return [("decoy", -1, None)] * 9 + [("plain075", None, 0.75)]
        return ([("planted", 0, None), ("decoy2", -1, None), ("plain0875", None, 0.875)]
                + ([("plain125", None, 1.25)] if i % 3 == 0 else []))
    return _defer_assemble(d, "floor", F16_MID, entries, nr, seed)


def defer_radius_case(d, nr=DEFER_NR, seed=3):
    """Rows 0..31: 4 plain 1.25 rows and 6 decoys one step larger (s_u) each: the event at row 32 sets the radius to s_u,
    the 128 plain rows stay and their score is the floor.  Rows 32..223: the partner (s < s_u = radius, its fp16 score
    ~0.9 eps above s: not provably > radius) and on every second row a plain 1.125 row (deferred)."""
    def entries(i):
        if i < 32:
            return [("plain125", None, 1.25)] * 4 + [("decoy_up", 1, None)] * 6
        return [("planted", 0, None)] + ([("plain1125", None, 1.125)] if i % 2 == 0 else [])
    return _defer_assemble(d, "radius", F16_MID_UP, entries, nr, seed)


def defer_deferrable(c):
    """the role a correct band defers, all of it and nothing else"""
    return "plain0875" if c.side == "floor" else "plain1125"


def score_matrix(c):
    """fp32 scores of all pairs: the chain score of every role's pairs; every other pair (random signs against random
    signs, far below every threshold of the schedule) by a float64 product rounded once.  Returns S and the mask of the
    role pairs."""
    S = (c.q.astype(np.float64) @ c.r.astype(np.float64).T).astype(np.float32)
    role = np.zeros(S.shape, bool)
    for rows, refs in c.roles.values():
        S[rows, refs] = chain(c.q[rows], c.r[refs])
        role[rows, refs] = True
    return S, role


def replay_schedule(S, K):
    """the reference's schedule on a score matrix (range_search_max_results: batches of 32, 64, ... rows, an event when
    more than 2K hits are kept): [(rows seen, kept before the event's test, event?, radius behind the boundary)]"""
    radius, kept, out, bs, i0 = np.float32(-1e10), np.empty(0, np.float32), [], 32, 0
    while i0 < len(S):
        i1 = min(len(S), i0 + bs)
        new = S[i0:i1].ravel()
        kept = np.concatenate([kept, new[new > radius]])
        n, event = len(kept), len(kept) > 2 * K
        if event:
            radius = np.sort(kept)[::-1][K]
            kept = kept[kept > radius]
        out.append((i1, n, event, radius))
        if bs < 20000:
            bs *= 2
        i0 = i1
    return out


def _edge(t, e):
    """prefilter_dev.h candidate_edge"""
    return (t - e) - 2.4e-7 * (np.abs(t) + e)


def defer_band(b, radius, floor, route, f_lo=1.0, f_hi=1.0):
    """The band of fp16 scores that the kernels defer, for the pairs of PairBound b: (candidate edge, lo, hi).
      route 'panel'   sim_f16p.hip defer_band: e = (radius - thr) 1.000001, thr = the column's candidate edge (bound of
                      the panel's largest query norm)
      route 'screen'  rescore.hip f16_screen_kernel: e = the pair's own eps
      lo = (radius + e) + 2.4e-7 (|radius| + e), hi = (floor - e) - 2.4e-7 (|floor| + e)
    f_lo, f_hi scale e on one edge: what a wrong band would be (1: the kernels'; 0: no bound; -1: the wrong sign)."""
    radius, floor = np.float64(radius), np.float64(floor)
    if route == "panel":
        thr = _edge(radius, b.eps)
        e = (radius - thr) * 1.000001
    else:
        assert route == "screen", route
        thr = _edge(radius, b.eps_pair)
        e = b.eps_pair
    e_lo, e_hi = f_lo * e, f_hi * e
    return thr, (radius + e_lo) + 2.4e-7 * (abs(radius) + e_lo), _edge(floor, e_hi)


def defer_margins(c, rows, refs, radius, floor, route):
    """(low - lo) / eps and (hi - low) / eps of the pairs: how far inside the band's two edges the fp16 score lies, in
    units of the bound.  A pair is deferred iff the first is > 0 and the second >= 0; a pair with exact score outside
    (radius, floor] must have one of them below 0, and is `-m` eps away from being deferred wrongly."""
    b = PairBound(c, rows, refs)
    _, lo, hi = defer_band(b, radius, floor, route)
    eps = b.eps if route == "panel" else b.eps_pair
    return (b.low - lo) / eps, (hi - b.low) / eps


def defer_predicted(c, rows, refs, radius, floor, route, f_lo=1.0, f_hi=1.0):
    """which of the pairs the (possibly wrong, see defer_band) band defers: candidates whose fp16 score lies in it"""
    b = PairBound(c, rows, refs)
    thr, lo, hi = defer_band(b, radius, floor, route, f_lo, f_hi)
    return (b.low > thr) & (b.low > lo) & (b.low <= hi)
