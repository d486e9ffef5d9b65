"""CPU: the reference codec of the Temporal-Network context, host side -- the codec string is validated before any
device is needed, and the C ABI carries the new entry points."""
import ctypes

import numpy as np
import pytest


def _videos(n):
    from vsc2022_amd.vsc.index import VideoFeature

    rng = np.random.default_rng(0)
    return [VideoFeature(video_id=f"V{k}", timestamps=np.arange(4.0), feature=rng.standard_normal((4, 8)).astype(np.float32))
            for k in range(n)]


def test_unknown_tn_codec_is_refused_before_any_device_is_needed():
    from vsc2022_amd.engine import DeviceMatcher
    from vsc2022_amd.vsc.baseline.localization import LocalizationWithMetadata, VCSLLocalization, VCSLLocalizationMaxSim

    q, r = _videos(2), _videos(3)
    for cls in (VCSLLocalization, VCSLLocalizationMaxSim):
        with pytest.raises(NotImplementedError):
            cls(q, r, "TN", ref_codec="PQ16")

    class Loc(LocalizationWithMetadata):
        def localize(self, candidate):
            return []

    with pytest.raises(NotImplementedError):
        Loc(q, r, ref_codec="PQ16")
    rows = np.zeros((12, 8), np.float32)
    with pytest.raises(NotImplementedError):
        DeviceMatcher(rows, np.array([0, 4, 8, 12]), tn_codec="PQ16")


def test_tn_codec_entry_points_are_exported():
    from vsc2022_amd import _lib

    assert {"vsc_tn_create_codec", "vsc_tn_ref_bytes"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.vsc_tn_ref_bytes.restype is ctypes.c_int64 and len(L.vsc_tn_create_codec.argtypes) == 13
    assert L.vsc_tn_ref_bytes(None) == 0
    # argument checks come before the device: an unknown codec id is VSC_ERR_INVALID with or without a GPU
    off = np.zeros(1, np.int64)
    ctx = ctypes.c_void_p()
    rc = L.vsc_tn_create_codec(None, off.ctypes.data, 0, None, 0, off.ctypes.data, 0, 8, _lib.MEM_HOST, _lib.MEM_HOST, 7, 0,
                               ctypes.byref(ctx))
    assert rc == _lib.VSC_ERR_INVALID and not ctx.value
