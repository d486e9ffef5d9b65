"""SQfp16 codec, the parts that need no GPU: the codec strings, the ABI tables, and the row sets of the GPU tests."""
import os
import re

import numpy as np
import pytest

import codec_rows as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_codec_strings():
    from vsc2022_amd import _lib

    assert _lib.codec_id("Flat") == _lib.CODEC_FLAT == 0
    assert _lib.codec_id("SQfp16") == _lib.CODEC_SQFP16 == 1
    for other in ("IVF64,Flat", "SQ8", "PCA64,Flat", "flat", "sqfp16", "", None):
        with pytest.raises(NotImplementedError) as e:
            _lib.codec_id(other)
        assert "'Flat'" in str(e.value) and "'SQfp16'" in str(e.value)


@pytest.mark.parametrize("codec", ["IVF64,Flat", "SQ8", "PQ16"])
def test_unknown_codecs_raise_before_any_device_is_needed(codec):
    from vsc2022_amd.vsc.index import FlatIndex, VideoIndex

    with pytest.raises(NotImplementedError):
        VideoIndex(16, codec)
    with pytest.raises(NotImplementedError):
        FlatIndex(16, codec=codec)


def test_known_codecs_are_accepted_up_to_the_device():
    """"Flat" and "SQfp16" pass the string check: whatever stops the constructor on a machine without a GPU, it is
    not NotImplementedError."""
    from vsc2022_amd import _lib
    from vsc2022_amd.vsc.index import VideoIndex

    if os.path.exists(_lib.LIB_PATH) and _lib.device_count() > 0:
        for codec in ("Flat", "SQfp16"):
            assert VideoIndex(16, codec).index.codec == codec
        return
    for codec in ("Flat", "SQfp16"):
        with pytest.raises(Exception) as e:
            VideoIndex(16, codec)
        assert not isinstance(e.value, NotImplementedError)


def test_header_and_exports_hold_the_codec_entry_points():
    from vsc2022_amd import _lib

    header = open(os.path.join(ROOT, "include", "vscmi.h")).read()
    declared = set(re.findall(r"\b(vsc_[a-z0-9_]+)\s*\(", header))
    for name in ("vsc_index_create_codec", "vsc_index_add_f16", "vsc_index_reconstruct"):
        assert name in declared and name in _lib.EXPORTS
    assert set(_lib.EXPORTS) == {n for n in declared if n != "vsc_index_t"}
    assert re.search(r"#define VSC_CODEC_FLAT 0\b", header) and re.search(r"#define VSC_CODEC_SQFP16 1\b", header)


@pytest.mark.parametrize("d", [16, 100, 256, 512, 768])
def test_row_sets_exercise_the_rounding(d):
    x = cr.rows(3, 700, d)
    assert np.isfinite(x).all() and np.abs(x).max() <= 65504.0
    dx = cr.dec(x)
    h = x.astype(np.float16)
    sub = (np.abs(dx) < 2.0 ** -14) & (dx != 0)
    assert sub.sum() >= 4, "no subnormal halves"
    assert ((x != 0) & (dx == 0)).sum() >= 2, "nothing rounds to zero"
    # values that round up into the next binade: |dec| is a power of two above |x|
    up = (np.abs(dx) > np.abs(x)) & (np.frexp(np.abs(dx))[0] == 0.5) & (np.abs(x) >= 2.0 ** -14)
    assert up.sum() >= 4, "nothing rounds up to the next binade"
    # exact ties: x lies exactly half way between two halves; both parities of the lower neighbour's mantissa occur
    x64, h64 = x.astype(np.float64), h.astype(np.float64)
    other = np.nextafter(h, np.where(x64 > h64, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)).astype(np.float64)
    tie = (x64 != h64) & (np.abs(x64 - h64) == np.abs(other - x64))
    # (numpy chose the neighbour with the even mantissa)
    assert ((h[tie].view(np.uint16) & 1) == 0).all()
    down = int((np.abs(h64[tie]) < np.abs(x64[tie])).sum())  # towards zero
    upw = int((np.abs(h64[tie]) > np.abs(x64[tie])).sum())   # away from zero
    assert down >= 2 and upw >= 2, (down, upw)
    # a wrong rounding mode cannot reproduce dec: truncation and round-half-away differ on these rows
    toward_zero = np.where(np.abs(dx) > np.abs(x), np.nextafter(h, np.float16(0)), h)
    assert not np.array_equal(toward_zero.astype(np.float32), dx)


def test_ties_set_has_ties_after_rounding():
    q, r = cr.with_ties(5, 120, 600, 32)
    s = cr.dec(q[:40]).astype(np.float64) @ cr.dec(r).astype(np.float64).T
    vals, counts = np.unique(s.astype(np.float32), return_counts=True)
    assert (counts > 1).sum() > 100
