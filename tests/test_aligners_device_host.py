"""CPU: the host side of the on-device DTW / DP aligners (`on_device=True`): the default route is untouched, the
device models construct without a device and refuse what the kernels have no room for, the library exports the two
entry points, and the published cell bound is the header's."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["DTW", "DP", "HV"])
def test_default_models_are_the_host_classes(name):
    from vsc2022_amd.vcsl import aligners
    from vsc2022_amd.vcsl.vta import build_vta_model

    model = build_vta_model(name)
    assert type(model) is getattr(aligners, name)
    assert model.on_device is False
    # ... and still align on the host: an all-ones matrix is one box
    sims = np.ones((33, 70), dtype=np.float32)
    assert model.forward_sim([("a", sims)]) == [("a", getattr(aligners, name.lower())(sims))]


@pytest.mark.parametrize("name", ["DTW", "DP"])
def test_device_models_construct_without_a_device(name):
    from vsc2022_amd import _lib
    from vsc2022_amd.vcsl import aligners
    from vsc2022_amd.vcsl.vta import build_vta_model

    model = build_vta_model(name, on_device=True, min_sim=1, min_length=np.int64(4), concurrency=8)
    assert type(model) is getattr(aligners, name) and model.on_device is True and model.device is None
    assert type(model.config["min_sim"]) is float and type(model.config["min_length"]) is int
    assert model.params.method == {"DTW": _lib.ALIGN_DTW, "DP": _lib.ALIGN_DP}[name]
    assert (model.params.discontinue, model.params.min_length, model.params.min_sim, model.params.max_iou) == (3, 4, 1.0, 0.3)
    assert model.params.max_path == (10 if name == "DP" else 0)
    assert build_vta_model(name, on_device=True, device=1).device == 1


@pytest.mark.parametrize("name", ["DTW", "DP", "HV"])
@pytest.mark.parametrize("on_device", [False, True])
def test_unknown_arguments_raise_type_error(name, on_device):
    from vsc2022_amd.vcsl.vta import build_vta_model

    with pytest.raises(TypeError):
        build_vta_model(name, on_device=on_device, tn_top_k=5)
    if name == "DTW":
        with pytest.raises(TypeError):
            build_vta_model(name, on_device=on_device, max_path=3)


@pytest.mark.parametrize("name,kw", [("DP", dict(max_path=17)), ("DP", dict(max_path=-1)), ("DP", dict(discontinue=16)),
                                     ("DTW", dict(discontinue=16)), ("DTW", dict(discontinue=-1)), ("DP", dict(min_length=-1)),
                                     ("DTW", dict(min_length=-1))])
def test_parameters_beyond_the_kernels_raise_value_error(name, kw):
    from vsc2022_amd.vcsl.vta import build_vta_model

    with pytest.raises(ValueError):
        build_vta_model(name, on_device=True, **kw)
    build_vta_model(name, **kw)  # (the host models take them as before)


def test_the_limits_themselves_are_accepted():
    from vsc2022_amd.vcsl.vta import build_vta_model

    build_vta_model("DP", on_device=True, max_path=16, discontinue=15, min_length=0)
    build_vta_model("DP", on_device=True, max_path=0, discontinue=0)
    build_vta_model("DTW", on_device=True, discontinue=15, min_length=0)


def test_hv_has_no_device_form():
    from vsc2022_amd.vcsl.vta import build_vta_model

    with pytest.raises(NotImplementedError):
        build_vta_model("HV", on_device=True)
    assert build_vta_model("HV", on_device=False).on_device is False


def test_library_exports_the_entry_points():
    from vsc2022_amd import _lib

    assert {"vsc_tn_align", "vsc_align_forward_sim"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert hasattr(L, "vsc_tn_align") and hasattr(L, "vsc_align_forward_sim")


def test_constants_are_the_headers():
    import ctypes

    from vsc2022_amd import _lib

    header = open(os.path.join(ROOT, "include", "vscmi.h")).read()
    value = {k: int(v) for k, v in re.findall(r"#define (VSC_ALIGN_[A-Z_]+) (\d+)\b", header)}
    assert value == {"VSC_ALIGN_DTW": _lib.ALIGN_DTW, "VSC_ALIGN_DP": _lib.ALIGN_DP, "VSC_ALIGN_MAX_CELLS": _lib.ALIGN_MAX_CELLS}
    # the shapes the device suite aligns on the device fit, the one it expects to be refused does not
    assert 65 * 130 <= _lib.ALIGN_MAX_CELLS < 300 * 400
    # struct vsc_align_params: four int32, two doubles
    assert ctypes.sizeof(_lib.AlignParams) == 32 and _lib.AlignParams.min_sim.offset == 16


def test_rejected_parameters_at_the_c_abi():
    """VSC_ERR_INVALID before any device is touched."""
    import ctypes

    from vsc2022_amd import _lib

    one = np.zeros(16 * 4, dtype=np.int32)
    sims, off, l1 = np.zeros(1, np.float32), np.array([0, 1], np.int64), np.ones(1, np.int32)
    for bad in (dict(method=3), dict(method=0), dict(discontinue=16), dict(discontinue=-1), dict(max_path=17), dict(max_path=-1),
                dict(min_length=-1)):
        cfg = dict(dict(method=_lib.ALIGN_DP, discontinue=3, min_length=5, max_path=10), **bad)
        prm = _lib.AlignParams(cfg["method"], cfg["discontinue"], cfg["min_length"], cfg["max_path"], 0.2, 0.3)
        rc = _lib.lib().vsc_align_forward_sim(sims.ctypes.data, off.ctypes.data, l1.ctypes.data, l1.ctypes.data, 1, ctypes.byref(prm),
                                              one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, 0)
        assert rc == _lib.VSC_ERR_INVALID, bad
        with pytest.raises(ValueError):
            _lib.check(rc)
