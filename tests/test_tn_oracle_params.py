"""The C oracle of the Temporal Network (oracle/vsc_oracle_tn.c) against the networkx restatement
(oracle/vcsl_shim/vcsl/vta.py) over the whole accepted parameter range -- away from the two parameter sets of
tests/golden/g5_*.  The restatement is the authority; tests/test_gpu_tn_params.py trusts the C oracle on these inputs
because of this file.  Host only.
"""
import os
import sys

import numpy as np
import pytest

pytest.importorskip("networkx")

import tn_cases as tc

_SHIM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "vcsl_shim")


@pytest.fixture(scope="module")
def shim_tn():
    """oracle/vcsl_shim's `vcsl.vta.tn`, loaded with the shim first on sys.path as oracle/gen_golden.py does -- and
    without leaving a top-level `vcsl` behind for the tests that install the package's own under that name."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "vcsl" or k.startswith("vcsl.")}
    sys.path.insert(0, _SHIM)
    try:
        from vcsl.vta import tn
    finally:
        sys.path.remove(_SHIM)
        for k in [k for k in sys.modules if k == "vcsl" or k.startswith("vcsl.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    assert os.path.abspath(tn.__code__.co_filename).startswith(_SHIM)
    return tn


def test_state_edge_arithmetic():
    """58 query rows are the last whose working state fits the 150 KiB LDS-state limit at top 16 / step 64."""
    assert tc.state_bytes(58, 16, 64) == 152512 and tc.state_bytes(59, 16, 64) == 155136
    assert tc.state_bytes(58, 16, 64) <= 150 * 1024 < tc.state_bytes(59, 16, 64)
    # the figures of the launch-budget rule (LDS-tile buckets of 64 and 256 rows, 4096 and 24576 floats)
    assert tc.state_bytes(256, 8, 10) == 72000
    assert tc.state_bytes(256, 5, 10) + 4 * 24576 == 143488 and tc.state_bytes(256, 5, 5) + 4 * 24576 == 134336
    assert 158 * 1024 - (tc.state_bytes(256, 7, 10) + 4 * 24576) == 384


def test_generators_reach_their_edges():
    zeros = tc.signed_zero_cases()
    assert len(zeros) == 40 and all(2 <= m.shape[0] <= 40 and 2 <= m.shape[1] <= 200 for _, m in zeros)
    for _, m in zeros:
        z = m[m == 0]
        assert np.signbit(z).any() and not np.signbit(z).all()
    assert {m.shape for _, m in tc.thin_wide_cases()} == set(tc.THIN_WIDE_SHAPES) and len(tc.thin_wide_cases()) == 21
    for name, m in tc.thin_wide_cases():
        if not name.endswith("q0"):  # quantised: every row repeats a score, so the ref index decides inside its top-k
            assert all(len(np.unique(row)) < len(row) for row in m)
    assert [m.shape[0] for _, m in tc.state_edge_cases()] == [58] * 3 + [59] * 3 + [64] * 3 + [65] * 3


@pytest.mark.parametrize("kw", tc.PARAM_SETS, ids=tc.set_id)
def test_c_oracle_equals_networkx_restatement(orc, shim_tn, kw):
    n_boxes = full = 0
    for name, sims in tc.host_cases():
        want = shim_tn(sims, **kw)
        got = orc.tn(sims, **kw)
        assert got == want, (name, sims.shape, kw, got, want)
        full = max(full, len(want))
    # the floor the GPU test relies on, over ITS inputs (the C oracle alone: it has just been pinned on a subset)
    n_boxes = sum(len(orc.tn(sims, **kw)) for _, sims in tc.gpu_cases())
    assert n_boxes >= tc.box_floor(kw), n_boxes
    if kw.get("tn_max_step", 10) == 1:
        assert n_boxes == 0
    if kw == tc.FULL_BUFFER:
        assert full == orc.MAX_BOXES, "no matrix fills the box buffer"
