"""The constructions of tests/prefilter_bounds.py, checked on the CPU in float64 against the kernels' own arithmetic.

test_gpu_prefilter_bounds.py can only catch a bound that is too tight if its inputs bring the real error close to the
bound and put every planted pair close to its threshold.  These tests hold the constructions to that, without a GPU:
if a change to the quantisers, the bounds or the rows themselves lets the error drift away from the bound, they fail
here instead of leaving the GPU tests quietly toothless.
"""
import functools

import numpy as np
import pytest

import prefilter_bounds as pb

GPU_CASES = [("f16", 64, {}), ("f16", 512, {}), ("f16", 768, {}), ("f16", 1000, {}), ("i8", 64, {}), ("i8", 512, {}),
             ("i8", 1000, {}), ("i8", 128, dict(exclude=True)), ("i8", 256, dict(centre=True))]


def margin_factor(kind, d):
    return pb.I8_MARGIN if kind == "i8" else min(pb.I8_MARGIN, pb.F16_REACH[d])


@pytest.mark.parametrize("d", [64, 128, 512, 1000])
def test_int8_construction_reaches_the_bound(d):
    """E_x N'_y + (N'_x + E_x) E_y + c_acc N_x N_y (with the kernels' safety factors) bounds the planted pairs' error,
    and they use >= 97 % of it; the same query rows against the noise references use far less"""
    c = pb.topk_case("i8", d, nq=96, nr=4096)
    rows, refs = c.planted()
    reach = pb.PairBound(c, rows, refs).reach()[0]
    assert (reach < 1.0).all() and reach.min() >= pb.I8_REACH, (reach.min(), reach.max())
    noise = pb.PairBound(c, rows, rows + 700).reach()[0]
    assert np.abs(noise).max() < 0.5 * pb.I8_REACH


@pytest.mark.parametrize("d", sorted(pb.F16_REACH))
def test_fp16_construction_reaches_the_bound(d):
    """the planted pairs' fp16 error is >= 0.95 / 0.85 / 0.75 of c1 |q||r| at D = 64 / 512 / 768 (and 1000, padded
    to 1024), and below the whole bound"""
    c = pb.topk_case("f16", d, nq=96, nr=4096)
    rows, refs = c.planted()
    of_eps, of_c1 = pb.PairBound(c, rows, refs).reach()
    assert (of_eps < 1.0).all() and of_c1.min() >= pb.F16_REACH[d], (of_c1.min(), of_eps.max())


@pytest.mark.parametrize("kind,d,kw", GPU_CASES)
def test_every_gpu_case_reaches_the_bound(kind, d, kw):
    """the variants of the GPU tests (one excluded coordinate, a centred reference image) reach the bound as well:
    the excluded coordinate and the centre move the thresholds, not the error"""
    c = pb.topk_case(kind, d, nq=96, nr=4096, **kw)
    rows, refs = c.planted()
    b = pb.PairBound(c, rows, refs)
    got = b.reach()[0] if kind == "i8" else b.reach()[1]
    assert got.min() >= (pb.I8_REACH if kind == "i8" else pb.F16_REACH[d]), got.min()
    if kw:
        assert (np.abs(b.shift) > 0.0).all()


@pytest.mark.parametrize("kind,d,kw", GPU_CASES)
def test_planted_pairs_sit_within_the_margin_of_every_threshold(kind, d, kw):
    """For each query kind of the GPU tests, at the threshold the planted pairs meet there: low + f eps < threshold
    (minus everything else the kernels take off it), so a bound f eps would drop every one of them -- f = 0.9 for int8,
    the dimension's reach (<= 0.9) for fp16 -- while eps keeps them.  Range search: radius = nextafter(s, -inf); top-K
    and k-NN: the decoys' score s_d just below s."""
    for c in (pb.topk_case(kind, d, **kw), pb.knn_case(kind, d, 5, **kw)):
        rows, refs = c.planted()
        s = pb.chain(c.q[rows], c.r[refs])
        assert (s == s[0]).all()                                    # one chain score for every planted pair
        s_d = pb.chain(c.q[rows], pb.decoys(c, rows))
        assert (s_d == s_d[0]).all() and s_d[0] < s[0]
        b = pb.PairBound(c, rows, refs)
        f = margin_factor(kind, d)
        for t in (np.nextafter(s[0], np.float32(-np.inf)), s_d[0]):
            m = b.margin(t)
            assert (m > f).all() and (m < 1.0).all(), (float(t), m.min(), m.max(), f)


# ---------------------------------------------------------------- deferred rescoring (test_gpu_defer_bounds.py)
DEFER_DIMS = [64, 512, 1000]
DEFER_ROUTES = ["panel", "screen"]
# the event at row 32 keeps: floor case 288 decoys; radius case 128 plain rows.  Then, per later row: floor case the
# partner, a decoy, a plain 0.875 row and on every third row a plain 1.25 row; radius case a plain 1.125 row on every
# second row (the partner is at or below the radius)
DEFER_SCHEDULE = {"floor": [(32, True), (96, 501, False), (224, 928, True)],
                  "radius": [(32, True), (96, 160, False), (224, 224, False)]}


@functools.lru_cache(maxsize=None)
def defer_case(side, d):
    """the case, its score matrix and the scores of its roles, built once and never modified"""
    c = pb.defer_floor_case(d) if side == "floor" else pb.defer_radius_case(d)
    S, role = pb.score_matrix(c)
    s = {}
    for name, (rows, refs) in c.roles.items():
        v = S[rows, refs]
        assert (v == v[0]).all(), (name, v.min(), v.max())            # one fp32 chain score per role
        s[name] = v[0]
    for a in (c.q, c.r, S, role):
        a.setflags(write=False)
    return c, S, role, s


def defer_thresholds(side, s):
    """(radius, floor) behind the event at row 32"""
    return (s["plain075"], s["decoy"]) if side == "floor" else (s["decoy_up"], s["plain125"])


def defer_f(d):
    return min(pb.I8_MARGIN, pb.F16_REACH[d])


@pytest.mark.parametrize("d", DEFER_DIMS)
def test_round_up_rows_reach_the_bound_from_above(d):
    """F16_MID_UP: the fp16 score lies ABOVE the exact one by as much of the bound as F16_MID's lies below it"""
    c, _, _, _ = defer_case("radius", d)
    rows, refs = c.planted()
    of_eps, of_c1 = pb.PairBound(c, rows, refs).reach()
    want = {64: -0.96, 512: -0.88, 1000: -0.79}[d]
    assert (np.abs(of_eps - want) < 0.01).all(), (of_eps.min(), of_eps.max())
    assert (of_eps > -1.0).all() and of_c1.max() <= -pb.F16_REACH[d], (of_c1.max(), of_eps.min())
    c, _, _, _ = defer_case("floor", d)
    rows, refs = c.planted()
    of_eps = pb.PairBound(c, rows, refs).reach()[0]
    assert (np.abs(of_eps + want) < 0.01).all(), (of_eps.min(), of_eps.max())


@pytest.mark.parametrize("d", DEFER_DIMS)
@pytest.mark.parametrize("side", ["floor", "radius"])
def test_defer_case_schedule(side, d):
    """the reference's schedule on the case's chain scores: the events, kept counts and radii the case is built for"""
    c, S, role, s = defer_case(side, d)
    if side == "floor":
        assert s["decoy"] == s["decoy2"] and s["decoy"] < s["planted"]                    # s_d < s, strictly
        assert s["plain075"] < s["plain0875"] < s["decoy"] and s["planted"] < s["plain125"]
    else:
        assert s["planted"] < s["decoy_up"]                                               # s < s_u, strictly
        assert s["decoy_up"] < s["plain1125"] < s["plain125"]
    radius, floor = defer_thresholds(side, s)
    sch = pb.replay_schedule(S, c.K)
    want = DEFER_SCHEDULE[side]
    assert [(b[0], b[2]) for b in sch] == [(w[0], w[-1]) for w in want], sch
    assert [b[1] for b in sch[1:]] == [w[1] for w in want[1:]], sch
    assert sch[0][1] == 32 * c.r.shape[0] and sch[0][3] == radius and sch[1][3] == radius, sch
    # the floor: every rank the rule can pick among the hits kept at row 32 gives one score
    kept = S[:32][S[:32] > radius]
    assert len(kept) == (288 if side == "floor" else 128) and (kept == floor).all()
    if side == "floor":
        assert sch[2][3] == s["decoy"]                  # the event at row 224: the new radius is s_d = the floor
        # ... and it is decided by the scored hits whether or not the planted pairs and the second decoys are among
        # them: a band that wrongly defers those still sees K + 1 scores at or above the floor, and drops them with D
        rows, refs = c.pairs("planted", "decoy2", pb.defer_deferrable(c))
        A = S.copy()
        A[rows, refs] = -np.inf
        A = A[A > radius]
        assert (A >= floor).sum() >= c.K + 1 and (S > floor).sum() <= c.K, ((A >= floor).sum(), (S > floor).sum())
        assert (S > floor).sum() == 192 + 64
    else:
        assert sch[2][3] == radius and (S > radius).sum() == 128 + 96 <= c.K


@pytest.mark.parametrize("d", DEFER_DIMS)
@pytest.mark.parametrize("side", ["floor", "radius"])
def test_defer_case_placement(side, d):
    """the reference count is no multiple of the 64-column wave tile, and the last, partial tile holds planted pairs of
    the 64-row batch (a partial 128-row panel) and of the 128-row batch; both batches have planted pairs in interior
    tiles as well"""
    c, _, _, _ = defer_case(side, d)
    nr = c.r.shape[0]
    assert nr % 64 != 0 and c.q.shape[0] == pb.DEFER_NQ == 224
    rows, refs = c.planted()
    assert np.array_equal(rows, np.arange(32, 224))
    last = refs >= nr // 64 * 64
    for lo, hi in ((32, 96), (96, 224)):
        batch = (rows >= lo) & (rows < hi)
        assert (batch & last).any() and (batch & ~last).sum() >= 32


@pytest.mark.parametrize("route", DEFER_ROUTES)
@pytest.mark.parametrize("d", DEFER_DIMS)
@pytest.mark.parametrize("side", ["floor", "radius"])
def test_planted_pairs_sit_within_the_margin_of_the_band(side, d, route):
    """Both kernels' bands, restated: on the attacked edge the planted pairs (and the floor case's second decoys) miss
    the band by less than (1 - f) eps; every plain row is on its side of every edge by more than 10 eps; the band
    defers the plain 0.875 / 1.125 rows and nothing else."""
    c, S, role, s = defer_case(side, d)
    radius, floor = defer_thresholds(side, s)
    f = defer_f(d)
    attacked = ["planted", "decoy2"] if side == "floor" else ["planted"]
    for name in attacked:
        rows, refs = c.roles[name]
        m_lo, m_hi = pb.defer_margins(c, rows, refs, radius, floor, route)
        m, other = (m_hi, m_lo) if side == "floor" else (m_lo, m_hi)
        assert (m < 0.0).all() and (m > f - 1.0).all() and (other > 10.0).all(), (name, m.min(), m.max(), other.min())
        # the same, from the threshold: the fp16 score is between f eps and eps away from it, on the unprovable side
        b = pb.PairBound(c, rows, refs)
        eps = b.eps if route == "panel" else b.eps_pair
        away = (np.float64(floor) - b.low) / eps if side == "floor" else (b.low - np.float64(radius)) / eps
        assert (away > f).all() and (away < 1.0).all(), (name, away.min(), away.max(), f)
    for name, (rows, refs) in c.roles.items():
        later = rows >= 32
        got = pb.defer_predicted(c, rows[later], refs[later], radius, floor, route)
        assert got.all() if name == pb.defer_deferrable(c) else not got.any(), (name, got.sum())
        if name.startswith("plain") and later.any():
            m_lo, m_hi = pb.defer_margins(c, rows[later], refs[later], radius, floor, route)
            assert (np.minimum(np.abs(m_lo), np.abs(m_hi)) > 10.0).all(), (name, m_lo.min(), m_hi.min())
    # every other pair of the later batches is below the candidate edge (the fp16 score of sign patterns against each
    # other is within eps of the exact one)
    b = pb.PairBound(c, *c.planted())
    edge = pb.defer_band(b, radius, floor, route)[0].min()
    assert S[32:][~role[32:]].max() < edge - 10.0 * b.eps.max()


@pytest.mark.parametrize("route", DEFER_ROUTES)
@pytest.mark.parametrize("d", DEFER_DIMS)
@pytest.mark.parametrize("side", ["floor", "radius"])
def test_narrower_bands_defer_the_planted_pairs(side, d, route):
    """the wrong bands the GPU tests must catch -- e scaled by the construction's reach f, e = 0, and e with the
    wrong sign, on the attacked edge -- each hold every planted pair; the kernels' band holds none"""
    c, _, _, s = defer_case(side, d)
    radius, floor = defer_thresholds(side, s)
    rows, refs = c.planted()
    assert not pb.defer_predicted(c, rows, refs, radius, floor, route).any()
    for f in (defer_f(d), 0.0, -1.0):
        kw = dict(f_hi=f) if side == "floor" else dict(f_lo=f)
        assert pb.defer_predicted(c, rows, refs, radius, floor, route, **kw).all(), f


def test_tighter_bounds_are_not_bounds_here():
    """the planted pairs' error exceeds each too-tight bound the GPU tests must catch: the int8 bound without its
    (N'_x + E_x) E_y term, 0.9 of it, and the fp16 bound with c1 built on 2^-11 instead of 2^-10"""
    for d in (64, 512, 1000):
        c = pb.topk_case("i8", d, nq=96, nr=4096)
        rows, refs = c.planted()
        b = pb.PairBound(c, rows, refs)
        _, _, Eq, Nq, Nkq = pb.i8_quantise(c.q[:128], panel=True)
        _, _, Er, Nr, Nkr = pb.i8_quantise(c.r[refs])
        assert (b.err > pb.i8_eps(Eq, Nq, Nkq, 0.0 * Er, Nr, Nkr, d)).all()
        assert (b.err > 0.9 * b.eps).all()
    for d in sorted(pb.F16_REACH):
        c = pb.topk_case("f16", d, nq=96, nr=4096)
        rows, refs = c.planted()
        b = pb.PairBound(c, rows, refs)
        c1, c2, c3 = pb.f16_coefficients(d)
        nq = np.linalg.norm(c.q.astype(np.float64), axis=1).max() * 1.0005
        nr = np.linalg.norm(c.r[refs].astype(np.float64), axis=1) * 1.0005
        assert (b.err > ((c1 - 2.0 ** -11) * nq * nr + c2 * (nq + nr) + c3) * 1.001).all()
