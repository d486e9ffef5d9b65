"""The half-float store of DnS's attention fine descriptors (VSC_FINE_F16), the part that needs no GPU: the ABI is
declared and bound, the new entry point judges its arguments before it reads the context and under its own fixed text,
vsc_tn_set_fine still refuses the new state as an unknown kind, and `fine_codec="SQfp16"` is refused before any device
call wherever it cannot run.
"""
import inspect
import os
import re

import numpy as np
import pytest

import dns_fine_ref as ref
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_FINE_TEXT = "vsc_tn_set_fine: invalid argument (regions 1..16, fdim >= 1, kind VSC_FINE_ATT / VSC_FINE_BIN)"
SET_FINE_F16_TEXT = "vsc_tn_set_fine_f16: invalid argument (regions 1..16, fdim >= 1, src_f16 0 / 1)"


def test_header_declares_and_lib_binds_the_half_store():
    from vsc2022_amd import _lib

    header = open(os.path.join(ROOT, "include", "vscmi.h")).read()
    declared = set(re.findall(r"\b(vsc_[a-z0-9_]+)\s*\(", header))
    assert "vsc_tn_set_fine_f16" in declared and "vsc_tn_set_fine_f16" in _lib.EXPORTS
    assert re.search(r"#define VSC_FINE_F16 3\b", header)
    assert _lib.FINE_F16 == 3 and (_lib.FINE_ATT, _lib.FINE_BIN, _lib.FINE_BITS) == (0, 1, 2)
    assert _lib.lib().vsc_tn_set_fine_f16.argtypes is not None and len(_lib.lib().vsc_tn_set_fine_f16.argtypes) == 7


def test_arguments_are_judged_before_the_context_is_read():
    """The context pointer is the address of a zeroed host buffer: reading it as a context would find no device and no
    offsets.  Every refusal carries the one fixed text."""
    from vsc2022_amd import _lib

    L = _lib.lib()
    not_a_context = np.zeros(4096, np.uint8)
    rows = np.zeros(4096, np.float32)
    ctx, x = not_a_context.ctypes.data, rows.ctypes.data
    for regions, fdim, src_f16 in ((0, 20, 0), (17, 20, 0), (4, 0, 1), (4, 20, 2), (4, 20, -1), (-1, 20, 1)):
        assert L.vsc_tn_set_fine_f16(ctx, x, None, regions, fdim, src_f16, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID
        assert L.vsc_last_error().decode() == SET_FINE_F16_TEXT
    for src_f16 in (0, 1):
        assert L.vsc_tn_set_fine_f16(None, x, None, 4, 20, src_f16, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID
        assert L.vsc_last_error().decode() == SET_FINE_F16_TEXT
    # VSC_FINE_F16 is no kind of vsc_tn_set_fine, whose text is unchanged
    assert L.vsc_tn_set_fine(ctx, x, None, 4, 20, _lib.FINE_F16, _lib.MEM_HOST) == _lib.VSC_ERR_INVALID
    assert L.vsc_last_error().decode() == SET_FINE_TEXT
    assert not not_a_context.any()


# ---- refusals of the Python route -----------------------------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    from vsc2022_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was asked for before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "default_device", refuse)


def _loc(model, kind="att", **kw):
    from vsc2022_amd.vsc.baseline.dns_baseline import VCSLLocalizationDnS

    qc, rc, qf, rf = ref.class_inputs(kind)
    (qv, qfv), (rv, rfv) = ref.video_features(qc, qf, "Q"), ref.video_features(rc, rf, "R")
    return VCSLLocalizationDnS(model, qfv, rfv, qv, rv, model_type="TN", device="cpu", **kw)


def test_the_codec_is_listed_and_others_stay_unknown(no_device):
    from vsc2022_amd.vsc.baseline import dns_baseline

    assert dns_baseline.FINE_CODECS == ("bits", "SQfp16")
    for on_device in (False, True):
        with pytest.raises(ValueError, match="unknown fine_codec 'nibbles'"):
            _loc(dns_baseline.ChamferSimilarity("att"), on_device=on_device, fine_codec="nibbles")


def test_half_store_needs_on_device(no_device):
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity

    with pytest.raises(ValueError, match="on_device=True"):
        _loc(ChamferSimilarity("att"), on_device=False, fine_codec="SQfp16")


def test_a_binary_student_is_sent_to_bits(no_device):
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity

    with pytest.raises(ValueError, match='"bits"'):
        _loc(ChamferSimilarity("bin"), kind="bin", on_device=True, fine_codec="SQfp16")


def test_half_store_needs_the_chamfer_class_itself(no_device):
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity

    class Derived(ChamferSimilarity):
        pass

    for model in (helpers.dns_standin("att"), Derived("att")):
        with pytest.raises(ValueError, match="ChamferSimilarity"):
            _loc(model, on_device=True, fine_codec="SQfp16")


def test_cli_takes_the_codec_and_needs_on_device(no_device, monkeypatch, tmp_path):
    import torch

    from vsc2022_amd.vsc.baseline import dns_baseline

    need = ["--torchscript_path", "a", "--query_coarse_features", "b", "--ref_coarse_features", "c",
            "--query_fine_features", "d", "--ref_fine_features", "e", "--output_path", str(tmp_path / "out")]
    assert dns_baseline.parser.parse_args(need).fine_codec is None
    assert dns_baseline.parser.parse_args(need + ["--on_device", "--fine_codec", "SQfp16"]).fine_codec == "SQfp16"
    action = next(a for a in dns_baseline.parser._actions if a.dest == "fine_codec")
    assert tuple(action.choices) == dns_baseline.FINE_CODECS  # the parser follows the list

    def no_model(*a, **k):
        raise AssertionError("the model was loaded before the arguments were checked")

    monkeypatch.setattr(torch.jit, "load", no_model)
    with pytest.raises(ValueError, match="--on_device"):
        dns_baseline.main(dns_baseline.parser.parse_args(need + ["--fine_codec", "SQfp16"]))


def test_the_functions_pass_the_codec_through(no_device):
    """localize_and_verify hands the argument to the class -- its refusals come back -- and match takes it too; the
    defaults of both signatures are what they were."""
    from vsc2022_amd.vsc.baseline import dns_baseline
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity, VCSLLocalizationDnS

    for fn in (dns_baseline.localize_and_verify, dns_baseline.match, VCSLLocalizationDnS.__init__):
        prm = inspect.signature(fn).parameters
        assert prm["fine_codec"].default is None and prm["on_device"].default is False
    qc, rc, qf, rf = ref.class_inputs("att")
    (qv, qfv), (rv, rfv) = ref.video_features(qc, qf, "Q"), ref.video_features(rc, rf, "R")
    with pytest.raises(ValueError, match="on_device=True"):
        dns_baseline.localize_and_verify(ChamferSimilarity("att"), qfv, rfv, qv, rv, [], fine_codec="SQfp16")
    with pytest.raises(ValueError, match='"bits"'):
        dns_baseline.localize_and_verify(ChamferSimilarity("bin"), qfv, rfv, qv, rv, [], on_device=True, fine_codec="SQfp16")
