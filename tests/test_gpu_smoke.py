"""The driver's smoke() in a FRESH process.

A fresh process has no neighbouring allocations, so an out-of-bounds access of a device buffer
faults instead of landing in some other test's memory (this is how the walk past the hit arrays
after a kept-hit overflow was found; csrc/select.hip select_begin_kernel).
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_smoke_in_fresh_process():
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "smoke ok" in r.stdout


@pytest.mark.gpu
def test_parity_suites_with_poisoned_allocations():
    """VSC_POISON_ALLOC=1 fills every fresh device buffer with 0xFF (NaN scores, -1 indices): a kernel
    that consumes memory nobody wrote fails the bit-exact parity tests instead of passing on the
    zero-filled pages a fresh allocation usually has."""
    env = dict(os.environ, VSC_POISON_ALLOC="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "tests/test_gpu_search.py",
                        "tests/test_gpu_tn.py", "tests/test_gpu_edge_cases.py", "tests/test_gpu_golden.py"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


_PARITY = ["tests/test_gpu_search.py", "tests/test_gpu_edge_cases.py", "tests/test_gpu_golden.py", "-k", "not rccl_world1"]
_FORCED_F16 = dict(VSC_PREFILTER="2", VSC_I8="0", VSC_TEST_QUICK="1")
_FORCED_I8 = dict(VSC_PREFILTER="2", VSC_I8="2", VSC_I8_CENTER="2", VSC_TEST_QUICK="1")
# family -> (route switches, pytest arguments): per kernel the smallest oracle-checked cases, nothing at full size and no
# test that starts a process of its own (profiles/stale_memory.md holds each family's time against the run above)
POISONED_FAMILIES = {
    "fp16-panel": (_FORCED_F16, _PARITY),
    "fp16-ring": (dict(_FORCED_F16, VSC_F16_KERNEL="ring"), _PARITY),
    "int8": (_FORCED_I8, _PARITY),
    "int8-screen-deferral": (dict(_FORCED_I8, VSC_I8_SCREEN="1", VSC_DEFER="2"),
                             ["tests/test_gpu_search.py", "tests/test_gpu_defer.py", "-k",
                              "test_gpu_search or forced_deferral or ties_on_radius"]),
    "codec": ({}, ["tests/test_gpu_codec.py", "-k", "every_route_equals_flat or store_holds_dec"]),
    "candidates": ({}, ["tests/test_gpu_pair_agg.py", "tests/test_gpu_search.py", "-k", "every_column or pair_max"]),
    "localisation": ({}, ["tests/test_gpu_tn_params.py", "tests/test_gpu_tn_codec.py", "-k",
                          "not (bytes_halve or cannot_hold or classes_take_ref_codec or out_of_range or Flat-0.0)"]),
    "aligners-rows-metric": ({}, ["tests/test_gpu_aligners_device.py", "tests/test_gpu_match_rows.py", "tests/test_gpu_match_metric.py",
                                  "-k", "host_function or thin_pairs or test_gpu_match_rows or coarse or lds_budget"]),
    "select-abi": ({}, ["tests/test_gpu_select_abi.py"]),
    # (one matcher over several query sets with half-float references only: with both codecs the file takes longer than the
    # run above, and the localisation family runs the Flat context under poison)
    "lifetime": ({}, ["tests/test_gpu_lifetime.py", "-k", "not (l5_one_matcher and Flat)"]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(POISONED_FAMILIES))
def test_kernel_families_with_poisoned_allocations(family):
    """The run above keeps to the default routes, which at its sizes is the exact fp32 kernel.  Here, under the same
    VSC_POISON_ALLOC=1: the fp16 panel and ring pre-filters, the int8 pre-filter, the fp16 screen, the exact stage with its
    candidate lists (shared tail and deferred set included), the SQfp16 store and its decoded ranges, the candidate
    aggregation, the Temporal Network's HBM state and half-float references, the aligners, the match rows, the segment
    AP, the scratch of the selection entry points -- and tests/test_gpu_lifetime.py, where handles are reused.  An
    unwritten index reads as -1 and an unwritten score as NaN: a reader of memory nobody wrote fails its parity test."""
    switches, args = POISONED_FAMILIES[family]
    env = dict(os.environ, VSC_POISON_ALLOC="1", **switches)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu"] + args, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_overflow_retry_in_fresh_process():
    """First search of the process overflows the default kept-hit buffer and is rerun with a larger
    one: results must still be the exact top-K prefix."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import oracle as orc
from vsc2022_amd.vsc.index import FlatIndex
rng = np.random.default_rng(5)
R = rng.standard_normal((900, 64)).astype(np.float32)
Q = rng.standard_normal((300, 64)).astype(np.float32)
idx = FlatIndex(64); idx.add(R)
# 32 rows x 900 refs = 2K exactly: the first batch does not re-threshold, the second one (64 rows)
# pushes the kept list to 86400 > the default buffer of 4K + 1024 = 58624 entries
K = 14400
i, j, s, rad = idx.global_topk(Q, K)
oi, oj, os_ = orc.global_threshold_search(Q, R, K)
assert np.array_equal(i, oi) and np.array_equal(j, oj)
assert np.array_equal(s.view(np.uint32), os_.view(np.uint32))
print("overflow ok", len(s))
""" % (ROOT, os.path.join(ROOT, "oracle"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "overflow ok" in r.stdout
