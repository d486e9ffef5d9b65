"""The constructions of tests/prefilter_bounds.py, checked on the CPU in float64 against the kernels' own arithmetic.

test_gpu_prefilter_bounds.py can only catch a bound that is too tight if its inputs bring the real error close to the
bound and put every planted pair close to its threshold.  These tests hold the constructions to that, without a GPU:
if a change to the quantisers, the bounds or the rows themselves lets the error drift away from the bound, they fail
here instead of leaving the GPU tests quietly toothless.
"""
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
