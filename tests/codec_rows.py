"""Row sets for the SQfp16 codec tests (tests/test_codec_host.py checks them, tests/test_gpu_codec.py uses them).

`dec(X)` is what an SQfp16 index stores: the rows rounded to IEEE half floats (round to nearest even, subnormals kept)
and converted back.  The rows below are descriptor-like (unit-norm Gaussian) with, planted into every row set, the
values on which a wrong rounding differs from numpy's `astype(float16)`:
  * halves in the SUBNORMAL range (|x| < 2^-14), including values below the smallest subnormal's half (-> 0);
  * values that round UP into the next binade (0.99999 -> 1.0, 1.9999 -> 2.0);
  * exact TIES between two neighbouring halves, with an even and with an odd lower neighbour (round to even goes down
    for one and up for the other; truncation, round-half-up and round-half-away all miss one of them).
"""
import numpy as np

# (value, what it is)
SPECIAL = (
    (np.float32(3.0e-6), "subnormal"), (np.float32(-4.5e-7), "subnormal"), (np.float32(2.0 ** -24 * 1.5), "subnormal tie"),
    (np.float32(2.0 ** -25), "tie with zero"), (np.float32(2.0 ** -26), "below half the smallest subnormal"),
    (np.float32(0.99999), "next binade"), (np.float32(-1.9999), "next binade"), (np.float32(0.2499999), "next binade"),
    (np.float32(1.0 + 2.0 ** -11), "tie, even below"), (np.float32(1.0 + 3 * 2.0 ** -11), "tie, odd below"),
    (np.float32(-(0.5 + 2.0 ** -12)), "tie, even below"), (np.float32(-(0.5 + 3 * 2.0 ** -12)), "tie, odd below"),
)


def dec(x):
    return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))


def rows(seed, n, d, special=True):
    """[n, d] fp32 unit-norm Gaussian rows; every SPECIAL value appears in row (7 m) % n at coordinate m % d, m =
    0, 1, ... (several rows each, so that small adds hold some too)."""
    rng = np.random.default_rng(seed)
    x = unit(rng, n, d)
    if special:
        for m in range(min(4 * len(SPECIAL), n)):
            x[(7 * m) % n, m % d] = SPECIAL[m % len(SPECIAL)][0]
    return x


def with_ties(seed, nq, nr, d):
    """(q, r) whose score matrix holds many exact ties, as oracle/gen_golden.py builds g2_search_ties: runs of identical
    rows (static scenes) inside the sets and a block of references duplicated elsewhere, so that the K cut of a
    global top-K falls inside a group of equal scores."""
    q, r = rows(seed, nq, d), rows(seed + 1, nr, d)
    for a in range(0, nr - 8, 37):
        r[a + 1:a + 4] = r[a]
    for a in range(0, nq - 6, 23):
        q[a + 1:a + 3] = q[a]
    blk = max(1, nr // 10)
    r[nr - blk:] = r[:blk]
    # planted copies: some query rows are (noisy) reference rows, so that the top of the score list is far above the rest
    for a in range(0, nq, 5):
        q[a] = r[(11 * a) % nr]
    return np.ascontiguousarray(q), np.ascontiguousarray(r)
