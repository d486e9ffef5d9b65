"""GPU parity of the Temporal-Network kernel over its whole accepted parameter range (tn_top_k 1..16, tn_max_step
1..64, max_path 0..15, any min_sim / max_iou): boxes equal to the CPU oracle's, list for list, and in the fused route
the similarity bits, MaxSim score bits and timestamps as well.  tests/test_tn_oracle_params.py pins the oracle to the
networkx restatement on the same inputs (tests/tn_cases.py).
"""
import functools

import numpy as np
import pytest

import tn_cases as tc
from codec_rows import dec
from helpers import bits

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- 1. forward_sim, the grid
@pytest.mark.parametrize("kw", tc.PARAM_SETS, ids=tc.set_id)
def test_forward_sim_over_the_parameter_grid(gpu, orc, kw):
    """One call per parameter set over 150 random matrices, the thin-and-wide shapes on both sides of the top-k method
    switch (plain and with scores in quarters / eighths), signed zeros, and the row counts around the LDS / HBM state
    split of top 16 / step 64."""
    from vsc2022_amd.vcsl.vta import build_vta_model

    data = list(tc.gpu_cases())
    got = build_vta_model("TN", **kw).forward_sim(data)
    assert [g[0] for g in got] == [d[0] for d in data]
    n_boxes = most = 0
    for (name, sims), (_, boxes) in zip(data, got):
        exp = orc.tn(sims, **kw)
        assert boxes == exp, (name, sims.shape, kw, boxes, exp)
        n_boxes += len(exp)
        most = max(most, len(exp))
    print(f"{tc.set_id(kw)}: {n_boxes} boxes over {len(data)} matrices, at most {most} in one")
    assert n_boxes >= tc.box_floor(kw), n_boxes
    if kw == tc.FULL_BUFFER:
        assert most == 16, "no matrix fills the box buffer (VSC_TN_MAX_BOXES)"


# ------------------------------------------------------------------------ 2. LDS state and HBM state in the same call
def test_lds_and_hbm_state_in_one_call(gpu, orc):
    """At top 16 / step 64 a pair of 58 query rows keeps its state in LDS and one of 59 runs from the HBM state slab
    (tests/tn_cases.py has the arithmetic): one call holds both kinds, interleaved, next to short pairs."""
    from vsc2022_amd.vcsl.vta import build_vta_model

    kw = tc.TOP16_STEP64
    edge, rand = list(tc.state_edge_cases()), list(tc.rand_cases(40))
    data = []
    for k in range(len(edge)):   # 58, 64, 58, 64, ... 59, 65, ... rows, a short pair after each
        data += [edge[(k % 2) * 6 + k // 2], rand[k]]
    assert sorted(m.shape[0] for _, m in data[::2]) == [58] * 3 + [59] * 3 + [64] * 3 + [65] * 3
    assert tc.state_bytes(58, 16, 64) <= 150 * 1024 < tc.state_bytes(59, 16, 64)
    got = build_vta_model("TN", **kw).forward_sim(data)
    assert [g[0] for g in got] == [d[0] for d in data]
    n_boxes = {True: 0, False: 0}
    for (name, sims), (_, boxes) in zip(data, got):
        exp = orc.tn(sims, **kw)
        assert boxes == exp, (name, sims.shape, boxes, exp)
        if name.startswith("edge"):
            n_boxes[sims.shape[0] >= 59] += len(exp)
    assert n_boxes[False] >= 3 and n_boxes[True] >= 9, n_boxes   # (the two planted diagonals of every edge matrix)


# ---------------------------------------------------------------------------- 3. fused route at wide parameters
Q_LENS = (256, 64, 100, 30, 12, 45, 20, 59)
R_LENS = (96, 64, 50, 30, 80, 33)
# (query video, ref video, first query frame, first ref frame, frames) of the planted copies
PLANTS = ((0, 0, 100, 10, 70), (1, 1, 8, 5, 50), (2, 4, 30, 20, 40), (3, 3, 5, 4, 20), (7, 2, 20, 10, 30), (5, 5, 10, 4, 25))
FUSED_SETS = (dict(tn_top_k=8), dict(tn_top_k=16, tn_max_step=10, min_length=3), tc.TOP16_STEP64)
D = 64


@functools.lru_cache(maxsize=None)
def fused_rows():
    """(query feature arrays, ref feature arrays): unit rows, d = 64, with noisy copies of reference segments in the
    queries.  The 256 x 96 pair is the largest tile of the 256-row LDS bucket (24 576 floats); 64 x 64 the largest of
    the 64-row one."""
    rng = np.random.default_rng(4242)

    def unit(n):
        x = rng.standard_normal((n, D)).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    q, r = [unit(n) for n in Q_LENS], [unit(n) for n in R_LENS]
    for qv, rv, q0, r0, n in PLANTS:
        seg = r[rv][r0:r0 + n] + (0.3 / np.sqrt(D)) * rng.standard_normal((n, D)).astype(np.float32)
        q[qv][q0:q0 + n] = seg / np.linalg.norm(seg, axis=1, keepdims=True)
    for x in q + r:
        x.setflags(write=False)
    return tuple(q), tuple(r)


def _videos(feats, prefix):
    from vsc2022_amd.vsc.index import VideoFeature

    out = []
    for v, f in enumerate(feats):
        ts = np.stack([np.arange(len(f), dtype=np.float32), np.arange(1, len(f) + 1, dtype=np.float32)], axis=1)
        out.append(VideoFeature(video_id=f"{prefix}{v:06d}", timestamps=ts, feature=np.array(f)))
    return out


@functools.lru_cache(maxsize=None)
def fused_sims(orc, codec, bias):
    """Oracle similarity matrices of all pairs (shared by the parameter sets)."""
    q, r = fused_rows()
    rr = [dec(x) for x in r] if codec == "SQfp16" else r
    return {(a, b): orc.pair_sims(q[a], rr[b], bias) for a in range(len(q)) for b in range(len(r))}


@pytest.mark.parametrize("kw", FUSED_SETS, ids=tc.set_id)
@pytest.mark.parametrize("codec,bias", [("Flat", 0.0), ("Flat", 0.5), ("SQfp16", 0.5)])
def test_fused_localize_at_wide_parameters(gpu, orc, codec, bias, kw):
    """Descriptors -> similarity tile -> TN -> MaxSim score with a working state several times that of the default
    parameters.  At tn_top_k = 8 the 256-row state (72 000 B) and the 256 x 96 tile (98 304 B) together exceed the LDS
    of a launch: the pair must take the similarity slab.  At top 16 / step 10 the 256-row pair, at top 16 / step 64
    every pair of 59 rows or more, runs from the HBM state slab AND a similarity slab; the shorter ones keep LDS state,
    with their tile in LDS (64-row bucket) or, at step 64, in the slab."""
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim
    from vsc2022_amd.vsc.metrics import CandidatePair

    q, r = fused_rows()
    queries, refs = _videos(q, "Q"), _videos(r, "R")
    loc = VCSLLocalizationMaxSim(queries, refs, "TN", similarity_bias=bias, ref_codec=codec, **kw)
    assert loc.ref_codec == codec
    cands = [CandidatePair(a.video_id, b.video_id, 1.0) for a in queries for b in refs]
    got = loc.localize_all(cands)
    sims_of = fused_sims(orc, codec, bias)
    if codec == "SQfp16":  # (the rounding changes the scores: equality with the Flat context's would not hold)
        assert not np.array_equal(bits(sims_of[0, 0]), bits(fused_sims(orc, "Flat", bias)[0, 0]))
    exp, per_pair = [], {}
    for c in cands:
        a, b = int(c.query_id[1:]), int(c.ref_id[1:])
        sims = sims_of[a, b]
        assert np.array_equal(bits(loc.similarity(c)), bits(sims)), (a, b)
        found = orc.tn(sims, **kw)
        per_pair[a, b] = found
        for (x1, y1, x2, y2) in found:
            score = sims[x1:x2, y1:y2].max() - np.float32(bias)
            exp.append((c.query_id, c.ref_id, np.float32(score), queries[a].timestamps[x1][0], queries[a].timestamps[x2][1],
                        refs[b].timestamps[y1][0], refs[b].timestamps[y2][1]))
    # every planted copy is found by the oracle, the 256 x 96 and the 64 x 64 pair among them
    for qv, rv, q0, r0, n in PLANTS:
        assert any(x1 <= q0 + 5 and x2 >= q0 + n - 6 and y1 <= r0 + 5 and y2 >= r0 + n - 6
                   for (x1, y1, x2, y2) in per_pair[qv, rv]), (qv, rv, per_pair[qv, rv])
    assert len(got) == len(exp), (len(got), len(exp))
    for g, e in zip(got, exp):
        assert (g.query_id, g.ref_id) == (e[0], e[1])
        assert np.float32(g.score).view(np.uint32) == e[2].view(np.uint32), (g, e)
        assert (g.query_start, g.query_end, g.ref_start, g.ref_end) == e[3:], (g, e)


# ------------------------------------------------------------------------------------- 4. parameters out of range
@pytest.mark.parametrize("kw", [dict(tn_top_k=0), dict(tn_top_k=17), dict(tn_max_step=0), dict(tn_max_step=65)],
                         ids=tc.set_id)
def test_out_of_range_parameters_are_refused(gpu, kw):
    from vsc2022_amd.vcsl.vta import build_vta_model
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim
    from vsc2022_amd.vsc.metrics import CandidatePair

    with pytest.raises(ValueError):
        build_vta_model("TN", **kw).forward_sim(list(tc.rand_cases(40)[:3]))
    q, r = fused_rows()
    loc = VCSLLocalizationMaxSim(_videos(q[3:5], "Q"), _videos(r[3:4], "R"), "TN", **kw)
    with pytest.raises(ValueError):
        loc.localize_all([CandidatePair("Q000000", "R000000", 1.0)])
