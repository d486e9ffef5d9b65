"""CPU: what the Temporal-Network part of the C ABI (csrc/api_tn.hip) refuses before any device call -- the return code
and the whole `vsc_last_error` text of every refusal, the entry point's own name inside it included.  The entry points
share their checks (one parameter check, one shape check, one body behind `vsc_tn_localize` / `_fine` and
`vsc_tn_similarity` / `_fine`): a shared helper that reports under the wrong name, or a check that moved behind the
first device call, fails here without a GPU."""
import ctypes

import numpy as np
import pytest

from vsc2022_amd import _lib

INVALID = _lib.VSC_ERR_INVALID
TN_PARAMS_TEXT = "unsupported TN parameters (tn_top_k 1..16, tn_max_step 1..64, max_path 0..15)"
SHAPE_TEXT = "has a negative shape or a matrix shorter than lq * lr"
SET_FINE_TEXT = "vsc_tn_set_fine: invalid argument (regions 1..16, fdim >= 1, kind VSC_FINE_ATT / VSC_FINE_BIN)"

# two pairs, 2 x 3 and 1 x 4: the arrays every forward_sim row starts from (kept alive here: the rows hold addresses)
SIMS = np.zeros(10, np.float32)
OFF = np.array([0, 6, 10], np.int64)
LQ = np.array([2, 1], np.int32)
LR = np.array([3, 4], np.int32)
NBOX = np.zeros(2, np.int32)
BOXES = np.zeros((2, _lib.TN_MAX_BOXES, 4), np.int32)
BMAX = np.zeros((2, _lib.TN_MAX_BOXES), np.float32)
STATUS = np.zeros(2, np.int32)
PAIRS = np.zeros(2, np.int32)
FOFF = np.array([0, 6], np.int64)
OUT = np.zeros(16, np.float32)
NROWS = ctypes.c_int64(0)
TN_OK = _lib.TNParams(10, 5, 10, 5, 0.2, 0.3)
ALIGN_OK = _lib.AlignParams(_lib.ALIGN_DTW, 3, 5, 0, 0.2, 0.3)
# vsc_tn_set_fine judges `regions` without reading the context: any non-null address stands for one
NOT_READ = np.zeros(4096, np.uint8)


def _a(x):
    return x.ctypes.data


def _tn_forward(sims=SIMS, off=OFF, lq=LQ, lr=LR, n=2, prm=TN_OK):
    return ("vsc_tn_forward_sim", (None if sims is None else _a(sims), _a(off), _a(lq), _a(lr), n, ctypes.byref(prm), _a(NBOX),
                                   _a(BOXES), _a(BMAX), 0))


def _align_forward(sims=SIMS, off=OFF):
    return ("vsc_align_forward_sim", (None if sims is None else _a(sims), _a(off), _a(LQ), _a(LR), 2, ctypes.byref(ALIGN_OK),
                                      _a(NBOX), _a(BOXES), _a(BMAX), _a(STATUS), 0))


def _tn_params(**kw):
    cfg = dict(dict(tn_max_step=10, tn_top_k=5, max_path=10), **kw)
    return _lib.TNParams(cfg["tn_max_step"], cfg["tn_top_k"], cfg["max_path"], 5, 0.2, 0.3)


def _match_rows(nbox=NBOX, boxes=BOXES, pair_q=PAIRS, n_rows=NROWS):
    # (count-only form: no output array, capacity 0; no context -- these checks need none)
    return ("vsc_tn_match_rows", (None, _a(pair_q), _a(PAIRS), 2, _lib.MEM_HOST, _a(nbox), _a(boxes), _a(BMAX), _lib.MEM_HOST,
                                  None, None, None, None, 0, _lib.MEM_HOST, None if n_rows is None else ctypes.byref(n_rows)))


def _changed(a, index, value):
    b = a.copy()
    b[index] = value
    return b


BOX_COUNT_17 = _changed(NBOX, 1, 17)
ONE_BOX = _changed(NBOX, 0, 1)
NEGATIVE_CORNER = _changed(BOXES, (0, 0, 2), -1)
NEGATIVE_ORDINAL = _changed(PAIRS, 1, -1)
SHORT_OFF = np.array([0, 5, 9], np.int64)  # the first matrix one cell short of 2 x 3

# (id, (entry point, arguments), return code, vsc_last_error)
REFUSALS = [
    ("tn_forward_sim-null-arrays", _tn_forward(sims=None), INVALID, "vsc_tn_forward_sim: invalid argument"),
    ("tn_forward_sim-negative-n", _tn_forward(n=-1), INVALID, "vsc_tn_forward_sim: invalid argument"),
    ("tn_forward_sim-top_k-0", _tn_forward(prm=_tn_params(tn_top_k=0)), INVALID, "vsc_tn_forward_sim: " + TN_PARAMS_TEXT),
    ("tn_forward_sim-top_k-17", _tn_forward(prm=_tn_params(tn_top_k=17)), INVALID, "vsc_tn_forward_sim: " + TN_PARAMS_TEXT),
    ("tn_forward_sim-max_step-0", _tn_forward(prm=_tn_params(tn_max_step=0)), INVALID, "vsc_tn_forward_sim: " + TN_PARAMS_TEXT),
    ("tn_forward_sim-max_step-65", _tn_forward(prm=_tn_params(tn_max_step=65)), INVALID, "vsc_tn_forward_sim: " + TN_PARAMS_TEXT),
    ("tn_forward_sim-max_path--1", _tn_forward(prm=_tn_params(max_path=-1)), INVALID, "vsc_tn_forward_sim: " + TN_PARAMS_TEXT),
    ("tn_forward_sim-max_path-16", _tn_forward(prm=_tn_params(max_path=16)), INVALID, "vsc_tn_forward_sim: " + TN_PARAMS_TEXT),
    ("align_forward_sim-null-arrays", _align_forward(sims=None), INVALID, "vsc_align_forward_sim: invalid argument"),
    ("align_forward_sim-short-matrix", _align_forward(off=SHORT_OFF), INVALID, "vsc_align_forward_sim: pair 0 " + SHAPE_TEXT),
    ("tn_localize-no-context",
     ("vsc_tn_localize", (None, _a(PAIRS), _a(PAIRS), 2, _lib.MEM_HOST, ctypes.byref(TN_OK), 0.0, _a(NBOX), _a(BOXES), _a(BMAX),
                          _lib.MEM_HOST)), INVALID, "vsc_tn_localize: invalid argument"),
    ("tn_localize_fine-no-context",
     ("vsc_tn_localize_fine", (None, _a(PAIRS), _a(PAIRS), 2, _lib.MEM_HOST, _a(SIMS), _a(FOFF), _lib.MEM_HOST, 1,
                               ctypes.byref(TN_OK), 0.0, _a(NBOX), _a(BOXES), _a(BMAX), _lib.MEM_HOST)),
     INVALID, "vsc_tn_localize_fine: invalid argument"),
    ("tn_localize_fine-no-fine-slab",
     ("vsc_tn_localize_fine", (None, _a(PAIRS), _a(PAIRS), 2, _lib.MEM_HOST, None, _a(FOFF), _lib.MEM_HOST, 1,
                               ctypes.byref(TN_OK), 0.0, _a(NBOX), _a(BOXES), _a(BMAX), _lib.MEM_HOST)),
     INVALID, "vsc_tn_localize_fine: invalid argument (no fine slab)"),
    ("tn_align-no-context",
     ("vsc_tn_align", (None, _a(PAIRS), _a(PAIRS), 2, _lib.MEM_HOST, ctypes.byref(ALIGN_OK), 0.0, _a(NBOX), _a(BOXES), _a(BMAX),
                       _a(STATUS), _lib.MEM_HOST)), INVALID, "vsc_tn_align: invalid argument"),
    ("tn_fine_similarity-no-context",
     ("vsc_tn_fine_similarity", (None, _a(PAIRS), _a(PAIRS), 2, _lib.MEM_HOST, 0, _a(OUT), _a(FOFF), 16, _lib.MEM_HOST)),
     INVALID, "vsc_tn_fine_similarity: invalid argument"),
    ("tn_similarity-no-context", ("vsc_tn_similarity", (None, 0, 0, 0.0, _a(OUT), 16, None, None)),
     INVALID, "vsc_tn_similarity: invalid argument"),
    ("tn_similarity_fine-no-context",
     ("vsc_tn_similarity_fine", (None, 0, 0, 0.0, _a(SIMS), _lib.MEM_HOST, 1, _a(OUT), 16, None, None)),
     INVALID, "vsc_tn_similarity_fine: invalid argument"),
    ("tn_set_stream-no-context", ("vsc_tn_set_stream", (None, None, 1)), INVALID, "vsc_tn_set_stream: invalid argument"),
    ("tn_set_timestamps-no-context", ("vsc_tn_set_timestamps", (None, None, None, _lib.MEM_HOST)),
     INVALID, "vsc_tn_set_timestamps: invalid argument"),
    ("tn_set_fine-no-context", ("vsc_tn_set_fine", (None, None, None, 4, 20, _lib.FINE_ATT, _lib.MEM_HOST)), INVALID, SET_FINE_TEXT),
    ("tn_set_fine-regions-0", ("vsc_tn_set_fine", (_a(NOT_READ), None, None, 0, 20, _lib.FINE_ATT, _lib.MEM_HOST)),
     INVALID, SET_FINE_TEXT),
    ("tn_match_rows-box-count-17", _match_rows(nbox=BOX_COUNT_17), INVALID, "vsc_tn_match_rows: pair 1 has a box count of 17 (0..16)"),
    ("tn_match_rows-negative-corner", _match_rows(nbox=ONE_BOX, boxes=NEGATIVE_CORNER), INVALID,
     "vsc_tn_match_rows: pair 0 has a negative box corner"),
    ("tn_match_rows-negative-ordinal", _match_rows(pair_q=NEGATIVE_ORDINAL), INVALID,
     "vsc_tn_match_rows: pair 1 has video ordinal out of range"),
    ("tn_match_rows-null-n_rows", _match_rows(n_rows=None), INVALID, "vsc_tn_match_rows: invalid argument"),
]

# vsc_tn_forward_sim's shape check (the aligner's, under its own name): without it the kernel read outside the caller's slab
NEGATIVE_LQ = _changed(LQ, 1, -1)
NEGATIVE_LR = _changed(LR, 0, -3)
REFUSALS += [
    ("tn_forward_sim-negative-lq", _tn_forward(lq=NEGATIVE_LQ), INVALID, "vsc_tn_forward_sim: pair 1 " + SHAPE_TEXT),
    ("tn_forward_sim-negative-lr", _tn_forward(lr=NEGATIVE_LR), INVALID, "vsc_tn_forward_sim: pair 0 " + SHAPE_TEXT),
    ("tn_forward_sim-short-matrix", _tn_forward(off=SHORT_OFF), INVALID, "vsc_tn_forward_sim: pair 0 " + SHAPE_TEXT),
]


@pytest.mark.parametrize("call,rc,text", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refused_before_any_device_call(call, rc, text):
    L = _lib.lib()
    name, args = call
    assert getattr(L, name)(*args) == rc
    assert L.vsc_last_error().decode() == text


@pytest.mark.parametrize("kw", [dict(dim=0), dict(codec=7)], ids=["dim-0", "codec-7"])
def test_create_codec_refuses_and_hands_back_no_context(kw):
    L = _lib.lib()
    cfg = dict(dict(dim=20, codec=_lib.CODEC_FLAT), **kw)
    feat, off = np.zeros((4, 20), np.float32), np.array([0, 4], np.int64)
    out = ctypes.c_void_p(1)
    rc = L.vsc_tn_create_codec(_a(feat), _a(off), 1, _a(feat), 0, _a(off), 1, cfg["dim"], _lib.MEM_HOST, _lib.MEM_HOST, cfg["codec"], 0,
                               ctypes.byref(out))
    assert rc == INVALID
    assert L.vsc_last_error().decode() == "vsc_tn_create_codec: invalid argument"
    assert out.value is None
