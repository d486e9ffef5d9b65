"""Parameter sets and seeded similarity matrices for the Temporal-Network tests over the whole accepted parameter range
(tn_top_k 1..16, tn_max_step 1..64, max_path 0..15).  Not a test module.

tests/test_tn_oracle_params.py pins the C oracle (oracle/vsc_oracle_tn.c) to the networkx restatement
(oracle/vcsl_shim/vcsl/vta.py) on exactly these inputs; tests/test_gpu_tn_params.py then checks the kernel against the C
oracle on them.  P below is (tn_max_step - 1) * tn_top_k: the predecessor slots of a DP node.  The kernel evaluates
P <= 32 in half-wave passes and larger P in chunks of 64 lanes; tn_top_k > 8 selects the per-row top-k by wave
arg-best, as do rows of more than 128 columns when there are fewer than 16 of them.
"""
import functools

import numpy as np

PARAM_SETS = (
    # top 1 (no division by `top`), and max_step 1 (P = 0: no regular edge at all)
    dict(tn_top_k=1),
    dict(tn_top_k=1, tn_max_step=1),
    dict(tn_max_step=1),
    # P = 16: one row step
    dict(tn_max_step=2, tn_top_k=16, min_length=1),
    # P = 32 exactly, three shapes (even top in the half-wave pass)
    dict(tn_top_k=8, tn_max_step=5, min_length=2),
    dict(tn_top_k=16, tn_max_step=3, min_length=1),
    dict(tn_top_k=4, tn_max_step=9, min_length=2),
    # P = 36 with top > 8
    dict(tn_top_k=9, tn_max_step=5, min_length=2),
    # P = 64 / 72 / 65: one chunk exactly, and the first lanes of a second one
    dict(tn_top_k=8, tn_max_step=9),
    dict(tn_top_k=8, tn_max_step=10),
    dict(tn_top_k=13, tn_max_step=6, min_length=2),
    # P = 144 / 1008 / 189: many chunks
    dict(tn_top_k=16, tn_max_step=10, min_length=3),
    dict(tn_top_k=16, tn_max_step=64, min_length=3),
    dict(tn_top_k=3, tn_max_step=64),
    # box logic: a full box buffer, IoU bounds that accept everything / nothing, one extraction, loose thresholds
    dict(tn_top_k=5, tn_max_step=5, min_length=1, max_iou=1.1, max_path=15),
    dict(tn_top_k=5, tn_max_step=5, min_length=1, max_iou=0.0),
    dict(max_path=0, min_length=2),
    dict(tn_top_k=6, tn_max_step=8, min_sim=-1.0, min_length=0, max_iou=0.9, max_path=15),
    dict(tn_top_k=12, min_sim=0.6, min_length=2),
    dict(min_sim=0.0, min_length=1, tn_top_k=9, tn_max_step=5),
)

TOP16_STEP64 = dict(tn_top_k=16, tn_max_step=64, min_length=3)
FULL_BUFFER = dict(tn_top_k=5, tn_max_step=5, min_length=1, max_iou=1.1, max_path=15)
assert TOP16_STEP64 in PARAM_SETS and FULL_BUFFER in PARAM_SETS


def set_id(kw):
    return ",".join(f"{k.replace('tn_', '')}={v}" for k, v in kw.items()) or "defaults"


def box_floor(kw):
    """The fewest boxes a parameter set must find over gpu_cases() for a comparison of box lists to mean anything.
    tn_max_step = 1 leaves only source -> sink paths, which hold no frame: no box ever.  Everywhere else the ~75
    matrices of rand_sims that carry planted diagonals of 3..29 cells give a box each at the loosest settings; 25 is a
    third of that, and max_path = 0 (one extraction per matrix) and min_sim = 0.6 still have to reach it.  The host
    test asserts the same floor on the oracle's output, so the GPU test cannot meet it by accident."""
    return 0 if kw.get("tn_max_step", 10) == 1 else 25


def rand_sims(rng, trial):
    """Random matrix of up to 69 x 89: plain noise, planted diagonals, values rounded to quarters / eighths (exact
    ties), a constant bias -- by `trial % 6`.  (tests/test_gpu_tn.py draws its inputs from here.)"""
    lq = int(rng.integers(1, 70))
    lr = int(rng.integers(1, 90))
    mode = trial % 6
    sims = rng.normal(0, 0.12, size=(lq, lr)).astype(np.float32)
    if mode in (1, 3, 5):
        for _ in range(rng.integers(1, 4)):
            L = int(rng.integers(3, 30))
            q0 = int(rng.integers(0, max(1, lq - 2)))
            r0 = int(rng.integers(0, max(1, lr - 2)))
            for t in range(L):
                if q0 + t < lq and r0 + t < lr:
                    sims[q0 + t, r0 + t] = 0.8 + 0.2 * rng.random()
    if mode in (2, 3):
        sims = np.round(sims * 4) / 4
    if mode == 4:
        sims += 0.5
    if mode == 5:
        sims = np.round(sims * 8) / 8 + 0.5
    return sims.astype(np.float32)


# few long rows on both sides of the top-k method switch `lq >= 16 || lr <= 128` (lane per row / wave arg-best)
THIN_WIDE_SHAPES = ((1, 129), (2, 300), (8, 130), (15, 128), (15, 400), (16, 129), (12, 200))


def thin_wide(rng, lq, lr, quant):
    """Noise with one planted diagonal; rounded to 1/quant for quant 4 or 8, so that a row holds long runs of equal
    scores and the (sim desc, ref asc) order of its top-k is decided by the ref index."""
    sims = rng.normal(0, 0.12, size=(lq, lr)).astype(np.float32)
    r0 = int(rng.integers(0, max(1, lr - lq)))
    for t in range(min(lq, lr - r0)):
        sims[t, r0 + t] = 0.8 + 0.2 * rng.random()
    if quant in (4, 8):
        sims = np.round(sims * quant) / quant
    return sims.astype(np.float32)


def signed_zero(rng, lq, lr):
    """Scores rounded to quarters (most are zero), half of the zeros negated, 0.5 on every second diagonal cell:
    -0.0 and +0.0 are ONE score to the stable argsort of the reference, so the ref index alone orders them."""
    sims = (np.round(rng.normal(0, 0.12, size=(lq, lr)) * 4) / 4).astype(np.float32)
    sims[sims == 0] = 0.0
    neg = (sims == 0) & (rng.random((lq, lr)) < 0.5)
    sims[neg] = np.float32(-0.0)
    for t in range(0, min(lq, lr), 2):
        sims[t, t] = 0.5
    return sims


def signed_zero_shape(rng):
    return int(rng.integers(2, 41)), int(rng.integers(2, 201))


# At tn_top_k 16 / tn_max_step 64 the working state of a pair (tn_state_bytes_host in csrc/tn.hip, 16-bit indices) is
#   lq * (16*2 + 16*4 + 2*64*2 + 16*64*16/8 + 16*4 + 16*2*3 + 8*8)  + 10 (source node) + 256 (boxes), rounded up
#   = 2624 lq + 266 + alignment:  58 rows -> 152 512 B,  59 rows -> 155 136 B.
# The LDS-state limit of a launch is 150 KiB = 153 600 B: 58 is the last row count whose state lives in LDS, 59 the
# first that runs from the HBM state slab (tn_pair_kernel<int, true>).
STATE_EDGE_LQ = (58, 59, 64, 65)
STATE_EDGE_LR = (33, 40, 70)


def state_bytes(lq, top, ms, idx_bytes=2):
    """tn_state_bytes_host restated (the library does not export it), for the arithmetic above."""
    al = lambda b, a: (b + a - 1) // a * a
    n_nodes = 1 + lq * top
    b = al(lq * top * idx_bytes, 16)
    b += lq * top * 4 + lq * ms * idx_bytes * 2
    b = al(b, 16)
    b = al(b + (lq * top * ms * top + 31) // 32 * 4, 16)
    b = al(b + n_nodes * 4 + n_nodes * idx_bytes * 3, 16)
    b += 16 * 16 + lq * ((top + 1) // 2) * 8
    return al(b, 64)


def state_edge(rng, lq, lr):
    """Noise in eighths plus 0.5 with two planted diagonals: boxes at every parameter set, ties in the DP."""
    sims = (np.round(rng.normal(0, 0.12, size=(lq, lr)) * 8) / 8 + 0.5).astype(np.float32)
    for q0, r0, n in ((2, 1, 25), (lq - 30, lr - 28, 26)):
        for t in range(n):
            if 0 <= q0 + t < lq and 0 <= r0 + t < lr:
                sims[q0 + t, r0 + t] = 1.3 + 0.2 * rng.random()
    return sims.astype(np.float32)


def _frozen(cases):
    for _, m in cases:
        m.setflags(write=False)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def rand_cases(n):
    rng = np.random.default_rng(2024)
    return _frozen([(f"rand{t}", rand_sims(rng, t)) for t in range(n)])


@functools.lru_cache(maxsize=None)
def thin_wide_cases():
    rng = np.random.default_rng(2025)
    return _frozen([(f"thin{lq}x{lr}q{quant}", thin_wide(rng, lq, lr, quant))
                    for quant in (0, 4, 8) for lq, lr in THIN_WIDE_SHAPES])


@functools.lru_cache(maxsize=None)
def signed_zero_cases(n=40):
    rng = np.random.default_rng(2026)
    # the first shapes are fixed: rows beyond 128 columns with fewer than 16 of them (wave arg-best at any top), and both ends
    shapes = [(2, 2), (40, 200), (3, 150), (15, 129), (9, 200), (16, 130)]
    shapes += [signed_zero_shape(rng) for _ in range(n - len(shapes))]
    return _frozen([(f"zero{t}_{lq}x{lr}", signed_zero(rng, lq, lr)) for t, (lq, lr) in enumerate(shapes)])


@functools.lru_cache(maxsize=None)
def state_edge_cases():
    rng = np.random.default_rng(2027)
    return _frozen([(f"edge{lq}x{lr}", state_edge(rng, lq, lr)) for lq in STATE_EDGE_LQ for lr in STATE_EDGE_LR])


def host_cases():
    """What the oracle is pinned to the networkx restatement on (per parameter set)."""
    return rand_cases(40) + thin_wide_cases() + signed_zero_cases() + state_edge_cases()


def gpu_cases():
    """What the kernel is checked on against the oracle (per parameter set): host_cases() and 110 more random matrices
    (rand_cases(40) is a prefix of rand_cases(150): one seeded stream)."""
    return rand_cases(150) + thin_wide_cases() + signed_zero_cases() + state_edge_cases()
