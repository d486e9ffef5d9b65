"""The 1-bit store of DnS's binary fine descriptors (VSC_FINE_BITS), the part that needs no GPU: the ABI is declared and
bound, the new entry point refuses without a context under its own name, the identity the integer kernel rests on --
the fp32 chain over {-1, +1} equals D - 2 popcount(q xor r) -- holds for the CPU restatement bit for bit, the host's
per-video packing is numpy's little-endian packbits, and `fine_codec` is refused before any device call wherever it
cannot run.
"""
import os
import re

import numpy as np
import pytest

import dns_fine_ref as ref
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SET_FINE_TEXT = "vsc_tn_set_fine: invalid argument (regions 1..16, fdim >= 1, kind VSC_FINE_ATT / VSC_FINE_BIN)"
SET_FINE_BITS_TEXT = "vsc_tn_set_fine_bits: invalid argument (regions 1..16, fdim 1..16777216, packed 0 / 1)"


def test_header_declares_and_lib_binds_the_bit_store():
    from vsc2022_amd import _lib

    header = open(os.path.join(ROOT, "include", "vscmi.h")).read()
    declared = set(re.findall(r"\b(vsc_[a-z0-9_]+)\s*\(", header))
    assert "vsc_tn_set_fine_bits" in declared and "vsc_tn_set_fine_bits" in _lib.EXPORTS
    assert re.search(r"#define VSC_FINE_BITS 2\b", header)
    assert _lib.FINE_BITS == 2 and (_lib.FINE_ATT, _lib.FINE_BIN) == (0, 1)
    assert "follow-up" not in header[header.index("DnS localisation on the device"):]
    assert _lib.lib().vsc_tn_set_fine_bits.argtypes is not None


def test_refused_without_a_context_under_its_own_name():
    from vsc2022_amd import _lib

    L = _lib.lib()
    not_read = np.zeros(4096, np.uint8)
    for packed in (0, 1):
        assert L.vsc_tn_set_fine_bits(None, not_read.ctypes.data, None, 4, 20, packed, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID
        assert L.vsc_last_error().decode() == SET_FINE_BITS_TEXT
    # vsc_tn_set_fine keeps its text, and VSC_FINE_BITS is no kind of it (judged before the context is read)
    assert L.vsc_tn_set_fine(None, None, None, 4, 20, _lib.FINE_ATT, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID
    assert L.vsc_last_error().decode() == SET_FINE_TEXT
    assert L.vsc_tn_set_fine(not_read.ctypes.data, None, None, 4, 20, _lib.FINE_BITS, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID
    assert L.vsc_last_error().decode() == SET_FINE_TEXT


# ---- the identity ---------------------------------------------------------------------------------------------------

POP8 = np.array([bin(k).count("1") for k in range(256)], dtype=np.int64)


def popcount_matrix(q, r):
    """G [Lq, R, Lr, R] of the bit store, with numpy integer operations on np.packbits output alone."""
    (lq, regions, dim), lr = q.shape, r.shape[0]
    qp = np.packbits(q, axis=-1, bitorder="little").reshape(lq * regions, -1)
    rp = np.packbits(r, axis=-1, bitorder="little").reshape(lr * regions, -1)
    pop = POP8[qp[:, None, :] ^ rp[None, :, :]].sum(axis=2)
    g = (dim - 2 * pop).astype(F32) / F32(dim)
    assert g.dtype == F32
    return g.reshape(lq, regions, lr, regions)


def _identity_inputs(dim, case):
    rng = np.random.default_rng(1000 + dim)
    q, r = rng.random((5, 3, dim)) > 0.5, rng.random((4, 3, dim)) > 0.5
    if case == "zeros":
        q[:], r[:] = False, False
    elif case == "ones":
        q[:], r[:] = True, True
    elif case == "complementary":
        r[:] = ~q[:4]
    elif case == "identical":
        r[:] = q[:4]
    return q, r


@pytest.mark.parametrize("case", ["random", "zeros", "ones", "complementary", "identical"])
@pytest.mark.parametrize("dim", [1, 7, 8, 31, 32, 33, 64, 65, 512, 4096])
def test_the_chain_is_the_popcount(orc, dim, case):
    q, r = _identity_inputs(dim, case)
    want = ref.region_matrix(q, r, "bin")
    got = popcount_matrix(q, r)
    assert np.array_equal(helpers.bits(got), helpers.bits(want))
    if case == "complementary":
        assert all(got[i, a, i, a] == -1.0 for i in range(4) for a in range(3))
    if case in ("identical", "zeros", "ones"):
        assert got.max() == 1.0


# ---- the host's packing ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 7, 8, 9, 16, 33, 512])
def test_pack_fine_bits_is_little_endian_packbits(dim):
    from vsc2022_amd.vsc.baseline.dns_baseline import pack_fine_bits

    rng = np.random.default_rng(dim)
    x = rng.random((6, 4, dim)) > 0.5
    want = np.packbits(x, axis=-1, bitorder="little")
    for given in (x, x.astype(np.uint8), x.astype(np.int64), x.astype(F32)):
        got = pack_fine_bits(given)
        assert got.dtype == np.uint8 and got.shape == (6, 4, (dim + 7) // 8) and np.array_equal(got, want)
    assert pack_fine_bits(x[:0]).shape == (0, 4, (dim + 7) // 8)  # a video without frames
    d = dim - 1  # element d sits in bit d % 8 of byte d / 8
    one = np.zeros((1, 1, dim), dtype=bool)
    one[0, 0, d] = True
    assert pack_fine_bits(one)[0, 0, d // 8] == 1 << (d % 8) and pack_fine_bits(one).sum() == 1 << (d % 8)


# ---- refusals -------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    from vsc2022_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was asked for before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "default_device", refuse)


def _loc(model, **kw):
    from vsc2022_amd.vsc.baseline.dns_baseline import VCSLLocalizationDnS

    qc, rc, qf, rf = ref.class_inputs("bin")
    (qv, qfv), (rv, rfv) = ref.video_features(qc, qf, "Q"), ref.video_features(rc, rf, "R")
    return VCSLLocalizationDnS(model, qfv, rfv, qv, rv, model_type="TN", device="cpu", **kw)


def test_bits_needs_on_device(no_device):
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity

    with pytest.raises(ValueError, match="on_device=True"):
        _loc(ChamferSimilarity("bin"), on_device=False, fine_codec="bits")


def test_bits_needs_binary_descriptors(no_device):
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity

    with pytest.raises(ValueError, match="bin"):
        _loc(ChamferSimilarity("att"), on_device=True, fine_codec="bits")


def test_bits_needs_the_chamfer_class_itself(no_device):
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity

    class Derived(ChamferSimilarity):
        pass

    for model in (helpers.dns_standin("bin"), Derived("bin")):
        with pytest.raises(ValueError, match="ChamferSimilarity"):
            _loc(model, on_device=True, fine_codec="bits")


def test_unknown_codec_name(no_device):
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity

    for on_device in (False, True):
        with pytest.raises(ValueError, match="unknown fine_codec"):
            _loc(ChamferSimilarity("bin"), on_device=on_device, fine_codec="nibbles")


def test_cli_fine_codec_needs_on_device(no_device, monkeypatch, tmp_path):
    import torch

    from vsc2022_amd.vsc.baseline import dns_baseline

    need = ["--torchscript_path", "a", "--query_coarse_features", "b", "--ref_coarse_features", "c",
            "--query_fine_features", "d", "--ref_fine_features", "e", "--output_path", str(tmp_path / "out")]
    assert dns_baseline.parser.parse_args(need).fine_codec is None
    assert dns_baseline.parser.parse_args(need + ["--on_device", "--fine_codec", "bits"]).fine_codec == "bits"
    with pytest.raises(SystemExit):
        dns_baseline.parser.parse_args(need + ["--on_device", "--fine_codec", "nibbles"])

    def no_model(*a, **k):
        raise AssertionError("the model was loaded before the arguments were checked")

    monkeypatch.setattr(torch.jit, "load", no_model)
    with pytest.raises(ValueError, match="--on_device"):
        dns_baseline.main(dns_baseline.parser.parse_args(need + ["--fine_codec", "bits"]))


def test_the_functions_pass_fine_codec_through(no_device):
    """localize_and_verify hands the argument to the class -- its refusals come back -- and match takes it too."""
    import inspect

    from vsc2022_amd.vsc.baseline import dns_baseline
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity

    for fn in (dns_baseline.localize_and_verify, dns_baseline.match):
        assert inspect.signature(fn).parameters["fine_codec"].default is None
    qc, rc, qf, rf = ref.class_inputs("bin")
    (qv, qfv), (rv, rfv) = ref.video_features(qc, qf, "Q"), ref.video_features(rc, rf, "R")
    with pytest.raises(ValueError, match="on_device=True"):
        dns_baseline.localize_and_verify(ChamferSimilarity("bin"), qfv, rfv, qv, rv, [], fine_codec="bits")
    with pytest.raises(ValueError, match="bin"):
        dns_baseline.localize_and_verify(ChamferSimilarity("att"), qfv, rfv, qv, rv, [], on_device=True, fine_codec="bits")
