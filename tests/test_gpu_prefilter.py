"""fp16 pre-filter + exact re-scoring (csrc/sim_f16*.hip, rescore.hip) must be INVISIBLE in the results.

The thresholded searches evaluate the bulk of the score matrix in fp16 and hand to the exact fp32
stage every pair whose fp16 score plus a rigorous error bound exceeds the radius.  The candidate set is
a superset of the exact hit set, so hits, order and fp32 bit patterns must equal the CPU oracle's
(vsc/index.py:142-165 semantics) -- with the pre-filter chosen by the density rule, forced onto every
batch (VSC_PREFILTER=2) or switched off (VSC_PREFILTER=0).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def prefilter_options(mode, **more):
    """The explicit form of VSC_PREFILTER=<mode> (+ other switches): options of the handle, set while it is still empty
    (`FlatIndex(..., options=...)` -> vsc_index_set_option; VERDICT r05 item 9: no test mutates os.environ around a
    handle's creation any more).  mode None: the defaults."""
    opts = {} if mode is None else {"prefilter": int(mode)}
    opts.update(more)
    return opts


def search_stats(idx):
    import ctypes

    from vsc2022_amd import _lib

    c, h = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().vsc_index_search_stats(idx._h, ctypes.byref(c), ctypes.byref(h)))
    return c.value


def run_topk(q, r, K, mode):
    from vsc2022_amd.vsc.index import FlatIndex

    idx = FlatIndex(q.shape[1], options=prefilter_options(mode))
    idx.add(r)
    i, j, s, radius = idx.global_topk(q, K)
    return i, j, s, radius, search_stats(idx)


def assert_same(a, b):
    assert len(a[2]) == len(b[2]), (len(a[2]), len(b[2]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(bits(a[2]), bits(b[2]))


@pytest.mark.parametrize("mode", [None, "2"])
@pytest.mark.parametrize("nq,nr,d,K", [(700, 3000, 128, 900), (300, 1000, 512, 200), (1100, 5000, 40, 3000),
                                        (64, 257, 100, 50)])
def test_topk_with_prefilter_matches_oracle(gpu, orc, mode, nq, nr, d, K):
    rng = np.random.default_rng(nq + nr + d)
    q, r = unit(rng, nq, d), unit(rng, nr, d)
    got = run_topk(q, r, K, mode)
    oi, oj, os_, info = orc.global_threshold_search(q, r, K, 0, return_info=True)
    assert_same(got, (oi, oj, os_))
    assert np.float32(got[3]) == np.float32(info["radius"])
    if mode == "2":
        assert got[4] >= len(os_)  # the pre-filter really ran: candidates are a superset of the hits


def test_prefilter_with_ties_and_duplicates(gpu, orc):
    """Static videos: many identical rows => exact score ties sit on the re-threshold values."""
    rng = np.random.default_rng(11)
    r = unit(rng, 2000, 64)
    r[100:400] = r[100]  # 300 identical reference rows
    q = unit(rng, 600, 64)
    q[50:120] = q[50]
    q[300:330] = r[100]  # exact copies of the repeated reference row
    for mode in (None, "2", "0"):
        got = run_topk(q, r, 1500, mode)
        oi, oj, os_ = orc.global_threshold_search(q, r, 1500)
        assert_same(got, (oi, oj, os_))


def test_prefilter_unnormalised_and_extreme_rows(gpu, orc):
    """Rows of very different norms, rows fp16 cannot represent (|x| > 65504, inf, NaN), tiny rows."""
    rng = np.random.default_rng(12)
    q = rng.standard_normal((400, 96)).astype(np.float32) * rng.uniform(0.01, 30.0, (400, 1)).astype(np.float32)
    r = rng.standard_normal((1500, 96)).astype(np.float32) * rng.uniform(0.01, 30.0, (1500, 1)).astype(np.float32)
    r[7] *= 1e-6  # far below the fp16 subnormal range
    r[8, 3] = 1e6  # overflows fp16
    q[9, 0] = 7e4
    r[10, 5] = np.inf
    q[11, 2] = np.nan
    r[12] = 0.0
    for mode in (None, "2"):
        got = run_topk(q, r, 2500, mode)
        oi, oj, os_ = orc.global_threshold_search(q, r, 2500)
        assert_same(got, (oi, oj, os_))


def test_range_search_with_prefilter(gpu, orc):
    from vsc2022_amd.vsc.index import FlatIndex

    rng = np.random.default_rng(13)
    q, r = unit(rng, 500, 128), unit(rng, 2100, 128)
    for mode in (None, "0"):
        idx = FlatIndex(128, options=prefilter_options(mode))
        idx.add(r[:900])
        idx.add(r[900:])
        lims, D, I = idx.range_search(q, 0.25)
        olims, oD, oI = orc.range_search(q, r, 0.25)
        assert np.array_equal(lims, olims) and np.array_equal(I, oI)
        assert np.array_equal(bits(D), bits(oD))


def test_fp16_error_bound_holds(gpu, orc):
    """Empirical check of the analytic bound the pre-filter relies on: |fp16 score - exact score| stays far
    below c1 * |q| * |r| (c1 ~ 1.1e-3 at D = 512) on descriptor-like data."""
    rng = np.random.default_rng(14)
    q, r = unit(rng, 256, 512), unit(rng, 1024, 512)
    exact = orc.scores(q, r).astype(np.float64)
    approx = q.astype(np.float16).astype(np.float64) @ r.astype(np.float16).astype(np.float64).T
    assert np.abs(approx - exact).max() < 0.25 * 1.1e-3


def test_prefilter_equals_fp32_path_at_scale(gpu):
    """Larger than the oracle can check quickly: the two device routes must agree bit for bit."""
    rng = np.random.default_rng(15)
    q, r = unit(rng, 6000, 256), unit(rng, 60000, 256)
    a = run_topk(q, r, 40000, None)
    b = run_topk(q, r, 40000, "0")
    assert_same(a, b)
    assert a[3] == b[3]
    assert a[4] > 0 and b[4] == 0  # the default route used the pre-filter, the fp32 route did not


def run_knn(q, r, k, mode):
    from vsc2022_amd.vsc.index import FlatIndex

    idx = FlatIndex(q.shape[1], options=prefilter_options(mode))
    idx.add(r)
    D, I = idx.search(q, k)
    return D, I, search_stats(idx)


@pytest.mark.parametrize("nq,nr,d,k", [(300, 5000, 128, 1), (257, 3000, 512, 20), (64, 200, 40, 64), (1000, 9000, 64, 5)])
def test_knn_with_forced_prefilter_matches_oracle(gpu, orc, nq, nr, d, k):
    """k-NN through subset threshold -> fp16 pre-filter -> exact stage -> per-row cut (VSC_PREFILTER=2)."""
    rng = np.random.default_rng(nq + nr + k)
    q, r = unit(rng, nq, d), unit(rng, nr, d)
    r[10:40] = r[10]  # ties: equal scores must come out in ascending ref order
    q[5] = r[10]
    D, I, cand = run_knn(q, r, k, "2")
    oD, oI = orc.knn(q, r, k)
    assert np.array_equal(I, oI)
    assert np.array_equal(bits(D), bits(oD))
    assert cand >= nq * k  # the pre-filtered route really ran


def test_knn_prefilter_chosen_by_size_matches_oracle(gpu, orc):
    """Large enough (>= 4e9 pairs, >= 65536 refs) for the route to be taken without forcing it."""
    rng = np.random.default_rng(21)
    q, r = unit(rng, 62000, 32), unit(rng, 70000, 32)
    D, I, cand = run_knn(q, r, 3, None)
    oD, oI = orc.knn(q, r, 3)
    assert np.array_equal(I, oI) and np.array_equal(bits(D), bits(oD))
    assert cand >= 62000 * 3
    D0, I0, cand0 = run_knn(q, r, 3, "0")
    assert np.array_equal(I0, oI) and np.array_equal(bits(D0), bits(oD)) and cand0 == 0


def test_parity_suites_with_forced_prefilter():
    """All search/candidate parity suites again with the pre-filter on every batch."""
    env = dict(os.environ, VSC_PREFILTER="2", VSC_TEST_QUICK="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "tests/test_gpu_search.py",
                        "tests/test_gpu_edge_cases.py", "tests/test_gpu_golden.py", "tests/test_gpu_sharded.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_parity_suites_with_the_lds_ring_kernel():
    """`sim_f16_kernel` (csrc/sim_f16.hip: the 256x256 LDS-ring pre-filter, the route of dims > 512) forced onto
    every batch of every dimension (VSC_F16_KERNEL=ring VSC_PREFILTER=2, int8 off): same suites, same oracle."""
    env = dict(os.environ, VSC_PREFILTER="2", VSC_F16_KERNEL="ring", VSC_I8="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "tests/test_gpu_search.py",
                        "tests/test_gpu_edge_cases.py", "tests/test_gpu_golden.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("d,nq,nr,K,k", [(768, 520, 3000, 1500, 5), (600, 300, 2100, 700, 20), (1000, 260, 1300, 900, 1)])
def test_dims_above_512_through_the_ring_kernel_match_oracle(gpu, orc, d, nq, nr, K, k):
    """DINO descriptors are 768-d (docs/baseline_dino.md): dims > 512 take sim_f16_kernel; deterministic cases against
    the oracle, thresholded search and k-NN, ties included (int8 off so that the fp16 ring kernel is what runs)."""
    from vsc2022_amd.vsc.index import FlatIndex

    rng = np.random.default_rng(d)
    q, r = unit(rng, nq, d), unit(rng, nr, d)
    r[40:90] = r[40]
    q[17] = r[40]
    idx = FlatIndex(d, options=prefilter_options("2", i8=0))
    idx.profile(True)
    idx.add(r[:1000])
    idx.add(r[1000:])
    got = idx.global_topk(q, K)
    oi, oj, os_, info = orc.global_threshold_search(q, r, K, 0, return_info=True)
    assert_same(got, (oi, oj, os_))
    assert np.float32(got[3]) == np.float32(info["radius"])
    D, I = idx.search(q, k)
    Do, Io = orc.knn(q, r, k)
    assert np.array_equal(I, Io) and np.array_equal(bits(D), bits(Do))
    p = idx.profile_read()
    assert p["f16_launches"] > 0 and p["i8_launches"] == 0


@pytest.mark.parametrize("case", ["refs_subnormal", "both_subnormal", "mixed_elements", "mixed_rows"])
def test_fp16_subnormal_rows_next_to_the_radius(gpu, orc, case):
    """The error bound of the pre-filter (api.hip: c2 = 2^-25 sqrt(D) per unit of norm) assumes GRADUAL underflow
    in fp16: elements below 6.1e-5 keep an absolute error of 2^-25.  If v_mfma_f32_32x32x16_f16 flushed fp16
    subnormal inputs to zero the error would be the whole product (2^-14 sqrt(D) per unit of norm) and true hits
    would be filtered out.  Rows whose elements lie in [6e-8, 6e-5], K chosen so that the radius falls INTO their
    score range, pre-filter forced on every batch, hits bit-identical to the oracle."""
    rng = np.random.default_rng(len(case))
    d, nq, nr = 512, 192, 1500
    q, r = unit(rng, nq, d), unit(rng, nr, d)
    tiny = np.float32(3e-4)  # unit-row elements ~ 0.044 -> ~1.3e-5: deep in the fp16 subnormal range
    if case == "refs_subnormal":
        r *= tiny
    elif case == "both_subnormal":
        q *= tiny
        r *= tiny
    elif case == "mixed_elements":
        r[:, ::2] *= tiny       # every other coordinate subnormal, the rest normal
        q[:, 1::3] *= tiny
    else:
        r[::2] *= tiny          # subnormal and normal rows side by side in every tile
        q[::3] *= tiny
    h = r.astype(np.float16)
    sub = (np.abs(h) < 6.1e-5) & (h != 0)
    assert sub.mean() > 0.2, sub.mean()
    K = int(0.3 * nq * nr)      # the K-th best score sits inside the bulk of the (tiny) scores
    want = orc.global_threshold_search(q, r, K)
    got = run_topk(q, r, K, "2")
    assert got[4] > 0           # candidates went through the fp16 stage
    assert_same(got, want)
    # and the k-NN through per-row thresholds
    from vsc2022_amd.vsc.index import FlatIndex

    idx = FlatIndex(d, options=prefilter_options("2"))
    idx.add(r)
    D, I = idx.search(q, 7)
    Do, Io = orc.knn(q, r, 7)
    assert np.array_equal(I, Io) and np.array_equal(bits(D), bits(Do))


@pytest.mark.parametrize("seed,nq,nr,d,K", [(21, 3000, 20000, 64, 150000), (22, 2500, 33000, 128, 40000)])
def test_fast_emission_path_matches_oracle(gpu, orc, seed, nq, nr, d, K):
    """The radius search's lean emission (sim_f16p.hip emit_candidates_seg) runs only while a whole tile still fits
    the wave's private segment of the candidate list, i.e. with large hit buffers: raise the capacity so that a
    medium-sized search takes it (every batch through the pre-filter), planted near-copies make dense blocks."""
    from vsc2022_amd.vsc.index import FlatIndex

    rng = np.random.default_rng(seed)
    q, r = unit(rng, nq, d), unit(rng, nr, d)
    for row in rng.choice(nq, 60, replace=False):           # rows with hundreds of strong hits
        tgt = rng.choice(nr, 300, replace=False)
        r[tgt] = q[row] + 0.25 * rng.standard_normal((300, d)).astype(np.float32)
        r[tgt] /= np.linalg.norm(r[tgt], axis=1, keepdims=True)
    idx = FlatIndex(d, options=prefilter_options("2"))
    idx.set_hit_capacity(24_000_000)                        # 2048 segments of > 8192 entries
    idx.add(r)
    i, j, s, radius = idx.global_topk(q, K)
    oi, oj, os_, info = orc.global_threshold_search(q, r, K, 0, return_info=True)
    assert_same((i, j, s), (oi, oj, os_))
    assert np.float32(radius) == np.float32(info["radius"])
    assert search_stats(idx) >= len(os_)


@pytest.mark.parametrize("kernel", ["panel", "ring"])
def test_full_segment_continues_in_the_shared_tail(gpu, orc, kernel):
    """A wave whose private segment is full goes on in its chunk of the shared tail (cand_list.h: cand_reserve): pinned
    for the panel kernel and the LDS-ring kernel with a capacity derived from the launch plan (tests/helpers.py: full_segment_capacity)."""
    from helpers import full_segment_capacity, full_segment_case
    from vsc2022_amd.vsc.index import FlatIndex

    q, r, radius, tile_cands = full_segment_case()
    olims, oD, oI = orc.range_search(q, r, radius)
    assert len(oI) == tile_cands                            # the dense tile, nothing else
    ring = kernel == "ring"
    # (i8=0: the fp16 kernels also where a parity suite runs this file with the int8 kernel switched on)
    idx = FlatIndex(q.shape[1], options=prefilter_options("2", f16_kernel=1 if ring else 0, i8=0))
    assert idx.get_option("f16_kernel") == (1 if ring else 0)
    idx.set_hit_capacity(full_segment_capacity(len(q), len(r), ring, tile_cands, len(oI)))
    idx.add(r)
    lims, D, I = idx.range_search(q, radius)                # (an overflow of either list is an error here, not a rerun)
    assert np.array_equal(lims, olims) and np.array_equal(I, oI)
    assert np.array_equal(bits(D), bits(oD))
