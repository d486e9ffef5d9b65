"""GPU parity: Temporal-Network localisation kernel vs the CPU oracle (boxes exact, fp32 bit-exact)."""
import numpy as np
import pytest

from tn_cases import rand_sims  # (the generator moved there unchanged: the same 400 matrices)

pytestmark = pytest.mark.gpu


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("kw", [{}, dict(tn_max_step=5, min_length=4),
                                dict(tn_max_step=3, tn_top_k=2, min_length=1, max_path=3),
                                dict(tn_top_k=7, min_sim=0.05)])
def test_forward_sim_matches_oracle(gpu, orc, kw):
    """build_vta_model('TN').forward_sim == oracle tn on 400 random matrices (ties, plants, bias)."""
    from vsc2022_amd.vcsl.vta import build_vta_model

    rng = np.random.default_rng(0)
    data = [(f"p{t}", rand_sims(rng, t)) for t in range(400)]
    model = build_vta_model("TN", concurrency=16, **kw)
    got = model.forward_sim(data)
    assert [g[0] for g in got] == [d[0] for d in data]
    nboxes = 0
    for (name, sims), (_, boxes) in zip(data, got):
        exp = orc.tn(sims, **kw)
        assert boxes == exp, (name, sims.shape, boxes, exp)
        nboxes += len(exp)
    assert nboxes > 100


def test_forward_sim_large_matrices(gpu, orc):
    from vsc2022_amd.vcsl.vta import build_vta_model

    rng = np.random.default_rng(1)
    data = []
    for t, (lq, lr) in enumerate([(300, 280), (500, 40), (40, 700), (257, 129), (1, 500), (600, 1)]):
        sims = rng.normal(0, 0.1, size=(lq, lr)).astype(np.float32)
        for k in range(min(lq, lr) // 2):
            sims[k + min(lq, lr) // 4, k + min(lq, lr) // 5] = 0.9
        data.append((f"big{t}", sims))
    got = build_vta_model("TN", tn_max_step=5, min_length=4).forward_sim(data)
    for (name, sims), (_, boxes) in zip(data, got):
        assert boxes == orc.tn(sims, tn_max_step=5, min_length=4), name


def _videos(rng, n, d, lo, hi, cls, prefix):
    out = []
    for v in range(n):
        L = int(rng.integers(lo, hi + 1))
        ts = np.stack([np.arange(L, dtype=np.float32), np.arange(1, L + 1, dtype=np.float32)], axis=1)
        out.append(cls(video_id=f"{prefix}{v:06d}", timestamps=ts, feature=unit(rng, L, d)))
    return out


@pytest.mark.parametrize("bias,kw", [(0.0, dict(tn_max_step=5, min_length=4)), (0.5, dict(tn_max_step=5, min_length=4)),
                                     (0.0, {})])
def test_fused_localize_matches_oracle(gpu, orc, bias, kw):
    """Fused path (descriptors in HBM -> MFMA sims -> TN -> MaxSim score) vs oracle sims + oracle tn."""
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim
    from vsc2022_amd.vsc.index import VideoFeature
    from vsc2022_amd.vsc.metrics import CandidatePair

    rng = np.random.default_rng(42)
    d = 512
    queries = _videos(rng, 12, d, 5, 60, VideoFeature, "Q")
    refs = _videos(rng, 14, d, 5, 80, VideoFeature, "R")
    refs.append(_videos(rng, 1, d, 300, 300, VideoFeature, "RL")[0])   # spills out of the LDS tile budget
    queries.append(_videos(rng, 1, d, 280, 280, VideoFeature, "QL")[0])
    # plant copies
    for (qi, ri, q0, r0, L) in [(0, 1, 2, 3, 20), (3, 3, 0, 10, 30), (5, 7, 10, 0, 12), (12, 14, 100, 50, 120)]:
        q, r = queries[qi], refs[ri]
        L = min(L, len(q) - q0, len(r) - r0)
        seg = r.feature[r0:r0 + L] + 0.05 * rng.standard_normal((L, d)).astype(np.float32)
        q.feature[q0:q0 + L] = seg / np.linalg.norm(seg, axis=1, keepdims=True)
    loc = VCSLLocalizationMaxSim(queries, refs, "TN", similarity_bias=bias, **kw)
    cands = [CandidatePair(q.video_id, r.video_id, 1.0) for q in queries for r in refs]
    got = loc.localize_all(cands)
    # oracle
    exp = []
    for c in cands:
        q = loc.queries[c.query_id]
        r = loc.refs[c.ref_id]
        sims = orc.pair_sims(q.feature, r.feature, bias)
        assert np.array_equal(bits(loc.similarity(c)), bits(sims))
        for (x1, y1, x2, y2) in orc.tn(sims, **kw):
            score = sims[x1:x2, y1:y2].max() - np.float32(bias)
            exp.append((c.query_id, c.ref_id, np.float32(score), q.timestamps[x1][0], q.timestamps[x2][1],
                        r.timestamps[y1][0], r.timestamps[y2][1]))
    assert len(got) == len(exp) and len(exp) >= 4
    for g, e in zip(got, exp):
        assert (g.query_id, g.ref_id) == (e[0], e[1])
        assert np.float32(g.score).view(np.uint32) == e[2].view(np.uint32)
        assert (g.query_start, g.query_end, g.ref_start, g.ref_end) == e[3:]


def test_reference_localization_properties(gpu):
    """tests/test_localization.py:46-66 of the reference, seeded (all-default TN parameters)."""
    from sklearn.preprocessing import normalize
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim
    from vsc2022_amd.vsc.index import VideoFeature
    from vsc2022_amd.vsc.metrics import CandidatePair

    rng = np.random.default_rng(7)
    D = 64

    def feat(n):
        return normalize(rng.normal(size=(n, D)))

    a, b, c = feat(45), feat(30), feat(60)
    a[20:30, :] = c[30:40, :]
    mk = lambda i, f: VideoFeature(video_id=i, feature=f, timestamps=np.arange(f.shape[0]) * 1.0)
    loc = VCSLLocalizationMaxSim([mk(1, a)], [mk(2, b), mk(3, c)], "TN")
    assert len(loc.localize(CandidatePair(1, 2, 1.0))) == 0
    assert len(loc.localize(CandidatePair(1, 3, 2.0))) >= 1
    ms = loc.localize_all([CandidatePair(1, 2, 1.0), CandidatePair(1, 3, 2.0)])
    assert len(ms) >= 1 and all(m.query_id == 1 and m.ref_id == 3 for m in ms)


def test_dns_style_fine_similarity_and_custom_aligner_route(gpu):
    """a subclass that overrides `similarity` (the reference's VCSLLocalizationDnS,
    vsc/baseline/dns_baseline.py:108-163) and a user-supplied aligner object both run on the reference's route:
    matrices per pair -> model.forward_sim -> score per box."""
    import torch

    from vsc2022_amd.vcsl.vta import build_vta_model, register_vta_model
    from vsc2022_amd.vsc.baseline.dns_baseline import VCSLLocalizationDnS
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim
    from vsc2022_amd.vsc.index import VideoFeature
    from vsc2022_amd.vsc.metrics import CandidatePair

    rng = np.random.default_rng(9)
    R, Df, Dc, Lq, Lr = 4, 16, 32, 30, 40

    def unit(*shape):
        x = rng.standard_normal(shape).astype(np.float32)
        return x / np.linalg.norm(x, axis=-1, keepdims=True)

    qf, rf = unit(Lq, R, Df), unit(Lr, R, Df)
    qc, rc = unit(Lq, Dc), unit(Lr, Dc)
    qf[8:20], qc[8:20] = rf[15:27], rc[15:27]          # planted copy, in both descriptor sets
    ts = lambda n: np.stack([np.arange(n, dtype=np.float32), np.arange(1, n + 1, dtype=np.float32)], 1)
    Q = lambda f: [VideoFeature(video_id="Q1", timestamps=ts(Lq), feature=f)]
    Rf = lambda f: [VideoFeature(video_id="R1", timestamps=ts(Lr), feature=f)]

    class Chamfer(torch.nn.Module):  # stand-in for the DnS student: mean over query regions of the best ref region
        fg_type = "att"

        def forward(self, a, b):
            return torch.einsum("ird,jsd->ijrs", a, b).max(dim=3).values.mean(dim=2)

    loc = VCSLLocalizationDnS(Chamfer(), Q(qf), Rf(rf), Q(qc), Rf(rc), "TN", "cuda", tn_max_step=5, min_length=4,
                              similarity_bias=0.0)
    cand = CandidatePair("Q1", "R1", 1.0)
    sim = loc.similarity(cand)
    a, b = torch.from_numpy(qf), torch.from_numpy(rf)
    fine = ((Chamfer()(a, b) + Chamfer()(b, a).mT) / 2.0 / 2.0 + 0.5).numpy()
    want = np.sqrt(fine.clip(1e-7) * (qc @ rc.T).clip(1e-7))
    assert sim.shape == (Lq, Lr) and np.abs(sim - want).max() < 2e-6
    matches = loc.localize_all([cand])
    assert matches and any(m.query_start <= 9 and m.query_end >= 19 and m.ref_start <= 16 and m.ref_end >= 26
                           for m in matches)
    assert all(abs(m.score - (sim[int(m.query_start):int(m.query_end) - 1, int(m.ref_start):int(m.ref_end) - 1].max()))
               < 1e-6 for m in matches)

    # a user aligner behind build_vta_model / model_type
    class WholeMatrix:
        def __init__(self, concurrency=1, **kw):
            self.seen = []

        def forward_sim(self, data):
            self.seen += [name for name, _ in data]
            return [(name, [[0, 0, s.shape[0] - 1, s.shape[1] - 1]]) for name, s in data]

    register_vta_model("WHOLE", WholeMatrix)
    assert isinstance(build_vta_model("WHOLE"), WholeMatrix)
    with pytest.raises(NotImplementedError):
        build_vta_model("SPD")   # (VCSL's trained detector: not buildable here, vsc2022_amd/vcsl/aligners.py)
    obj = WholeMatrix()
    loc2 = VCSLLocalizationMaxSim(Q(qc), Rf(rc), obj)
    m2 = loc2.localize_all([cand])
    assert obj.seen == ["Q1-R1"] and len(m2) == 1 and (m2[0].query_start, m2[0].query_end) == (0.0, float(Lq))
    assert abs(m2[0].score - (qc @ rc.T)[: Lq - 1, : Lr - 1].max()) < 2e-6


def test_over_long_videos_run_from_hbm_state(gpu, orc):
    """Query videos whose working state exceeds the LDS, and references beyond 32767 frames (16-bit indices),
    take the HBM-state route of the same kernel: boxes equal to the oracle, next to ordinary pairs in one call."""
    from vsc2022_amd.vcsl.vta import build_vta_model

    rng = np.random.default_rng(7)
    data = []
    for t, (lq, lr) in enumerate([(1500, 90), (30, 33000), (40, 60), (2200, 2100)]):
        sims = rng.normal(0, 0.1, size=(lq, lr)).astype(np.float32)
        n = min(lq, lr)
        for k in range(n // 2):
            sims[k + n // 4, k + n // 5] = 0.9
        if t == 0:
            sims = (np.round(sims * 8) / 8).astype(np.float32)   # exact ties: the lazy topological order runs
        data.append((f"long{t}", sims))
    for kw in (dict(tn_max_step=5, min_length=4), {}):
        got = build_vta_model("TN", **kw).forward_sim(data)
        for (name, sims), (_, boxes) in zip(data, got):
            assert boxes == orc.tn(sims, **kw), (name, kw)
        assert sum(len(b) for _, b in got) >= 3


def test_fused_localize_over_long_video(gpu, orc):
    """Fused route (descriptors -> sims -> TN) with a 1400-frame query video: HBM state + similarity slab."""
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim
    from vsc2022_amd.vsc.index import VideoFeature
    from vsc2022_amd.vsc.metrics import CandidatePair

    rng = np.random.default_rng(8)
    d = 64
    queries = _videos(rng, 1, d, 1400, 1400, VideoFeature, "Q") + _videos(rng, 2, d, 20, 40, VideoFeature, "QS")
    refs = _videos(rng, 1, d, 900, 900, VideoFeature, "R") + _videos(rng, 2, d, 30, 50, VideoFeature, "RS")
    seg = refs[0].feature[100:500] + 0.05 * rng.standard_normal((400, d)).astype(np.float32)
    queries[0].feature[700:1100] = seg / np.linalg.norm(seg, axis=1, keepdims=True)
    kw = dict(tn_max_step=5, min_length=4)
    loc = VCSLLocalizationMaxSim(queries, refs, "TN", similarity_bias=0.5, **kw)
    cands = [CandidatePair(q.video_id, r.video_id, 1.0) for q in queries for r in refs]
    got = loc.localize_all(cands)
    exp = []
    for c in cands:
        q, r = loc.queries[c.query_id], loc.refs[c.ref_id]
        sims = orc.pair_sims(q.feature, r.feature, 0.5)
        for (x1, y1, x2, y2) in orc.tn(sims, **kw):
            exp.append((c.query_id, c.ref_id, np.float32(sims[x1:x2, y1:y2].max() - np.float32(0.5)),
                        q.timestamps[x1][0], q.timestamps[x2][1], r.timestamps[y1][0], r.timestamps[y2][1]))
    assert len(got) == len(exp) and len(exp) >= 1
    for g, e in zip(got, exp):
        assert (g.query_id, g.ref_id) == (e[0], e[1])
        assert np.float32(g.score).view(np.uint32) == e[2].view(np.uint32)
        assert (g.query_start, g.query_end, g.ref_start, g.ref_end) == e[3:]
