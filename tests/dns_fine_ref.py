"""CPU restatement of the DnS localisation arithmetic (include/vscmi.h, "DnS localisation on the device") and the inputs
the host and GPU tests of it share.

Every step is the oracle's fp32 fma chain (`oracle.pair_sims`), one correctly rounded numpy fp32 operation, or the
oracle's Temporal Network (`oracle.tn`): the device route has to return these BITS.
"""
import numpy as np

import oracle as orc

F32 = np.float32
REF_PARAMS = dict(tn_max_step=5, min_length=4)     # what the reference passes (dns_baseline.py:196-199)
SLAB_PARAMS = dict(tn_top_k=8, tn_max_step=10)     # the state of a 256-frame bucket no longer fits LDS beside its tile


def signed(x, kind):
    """Fine descriptors as the arithmetic sees them: att as fp32, bin {0, 1} as 2 x - 1."""
    if kind == "bin":
        return (2.0 * np.asarray(x).astype(F32) - 1.0).astype(F32)
    return np.ascontiguousarray(x, dtype=F32)


def region_matrix(q, r, kind):
    """Step 1: G [Lq, R, Lr, R], the chain over d ascending; bin: divided once by (float)D."""
    q, r = signed(q, kind), signed(r, kind)
    (lq, regions, dim), lr = q.shape, r.shape[0]
    g = orc.pair_sims(q.reshape(lq * regions, dim), r.reshape(lr * regions, dim))
    if kind == "bin":
        g = g / F32(dim)
    return g.reshape(lq, regions, lr, regions)


def fine_sim(q, r, kind, symmetric, g=None):
    """Steps 1-4: F [Lq, Lr] of one pair (g: its region matrix when the caller has it already)."""
    lq, regions, lr = len(q), q.shape[1], len(r)
    if lq == 0 or lr == 0:
        return np.zeros((lq, lr), dtype=F32)
    g = region_matrix(q, r, kind) if g is None else g
    assert g.dtype == F32
    fwd = g.max(axis=3)  # [Lq, a, Lr]
    t = np.zeros((lq, lr), dtype=F32)
    for a in range(regions):
        t = t + fwd[:, a, :]
    f0 = t / F32(regions)
    if symmetric:
        bwd = g.max(axis=1)  # [Lq, Lr, b]
        u = np.zeros((lq, lr), dtype=F32)
        for b in range(regions):
            u = u + bwd[:, :, b]
        f0 = (f0 + u / F32(regions)) / F32(2.0)
    out = f0 / F32(2.0) + F32(0.5)
    assert out.dtype == F32
    return out


def blend(fine, coarse):
    """Step 5 with geometric_mean: the reference's statement on fp32 arrays."""
    fine, coarse = np.asarray(fine, dtype=F32), np.asarray(coarse, dtype=F32)
    out = np.sqrt(fine.clip(1e-7) * coarse.clip(1e-7))
    assert out.dtype == F32
    return out


def localise(s, params, bias):
    """Step 6: (boxes, MaxSim scores as fp32) of one blended matrix."""
    if s.shape[0] == 0 or s.shape[1] == 0:
        return [], []
    boxes = orc.tn(s, **params)
    scores = [F32(s[x1:x2, y1:y2].max() - F32(bias)) for x1, y1, x2, y2 in boxes]
    return boxes, scores


def half_rounded(x):
    """dec(X) of an SQfp16 context."""
    return np.asarray(x, dtype=F32).astype(np.float16).astype(F32)


# ---- inputs -------------------------------------------------------------------------------------------------------

def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(F32)
    return (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)).astype(F32)


def planted(seed, q_lens, r_lens, dim, regions, fdim, kind, noise=0.03):
    """(coarse queries, coarse refs, fine queries, fine refs) as lists of arrays.  Query k holds a noisy copy of a run of
    frames of reference k % len(r_lens) (three quarters of the shorter video); the fine descriptors are projections of
    the coarse ones, as tests/helpers.py:g9_inputs derives them, so a copy shows in both."""
    rng = np.random.default_rng(seed)
    refs = [unit_rows(rng, n, dim) for n in r_lens]
    queries = []
    for k, n in enumerate(q_lens):
        q = unit_rows(rng, n, dim)
        r = refs[k % len(refs)]
        run = min(n, len(r)) * 3 // 4
        if run >= 1:
            a, b = int(rng.integers(0, n - run + 1)), int(rng.integers(0, len(r) - run + 1))
            x = r[b:b + run] + noise * rng.standard_normal((run, dim)).astype(F32)
            q[a:a + run] = x / np.linalg.norm(x, axis=1, keepdims=True)
        queries.append(q.astype(F32))
    proj = rng.standard_normal((regions, dim, fdim)).astype(F32)

    def fine(v):
        x = np.einsum("ld,rde->lre", v, proj) + 0.05 * rng.standard_normal((len(v), regions, fdim)).astype(F32)
        if kind == "bin":
            return x > 0
        return (x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)).astype(F32)

    return queries, refs, [fine(v) for v in queries], [fine(v) for v in refs]


# the planted inputs of the class tests (tests/test_dns_device_host.py checks on the CPU that no alignment decision of
# theirs hangs on a rounding; tests/test_gpu_dns_device.py runs them on the device)
CLASS_Q_LENS = (40, 25, 33, 12, 64)
CLASS_R_LENS = (50, 31, 20, 45)
CLASS_PAIRS = [(k, k % 4) for k in range(5)] + [(0, 1), (2, 0), (4, 3), (1, 1), (3, 0)]


def class_inputs(kind):
    return planted(41 if kind == "att" else 43, CLASS_Q_LENS, CLASS_R_LENS, 64, 4, 16, kind)


def video_features(coarse, fine, prefix):
    """VideoFeature lists (coarse, fine) with 1 s frames."""
    from vsc2022_amd.vsc.index import VideoFeature

    out_c, out_f = [], []
    for k, (c, f) in enumerate(zip(coarse, fine)):
        ts = np.stack([np.arange(len(c), dtype=F32), np.arange(len(c), dtype=F32) + 1], axis=1)
        out_c.append(VideoFeature(video_id=f"{prefix}{k:03d}", timestamps=ts, feature=c))
        out_f.append(VideoFeature(video_id=f"{prefix}{k:03d}", timestamps=ts, feature=f))
    return out_c, out_f


def torch_route_sim(model, q_fine, r_fine, coarse, symmetric, geometric_mean):
    """S of one pair as the host route of VCSLLocalizationDnS.similarity states it (torch on the CPU, numpy blend)."""
    import torch

    with torch.no_grad():
        q, r = torch.from_numpy(np.asarray(q_fine)).float(), torch.from_numpy(np.asarray(r_fine)).float()
        if "bin" in model.fg_type:
            q, r = 2 * q - 1, 2 * r - 1
        sim = model(q, r)
        if symmetric:
            sim = (sim + model(r, q).mT) / 2.0
        sim = (sim / 2.0 + 0.5).numpy()
    if geometric_mean:
        sim = np.sqrt(sim.clip(1e-7) * coarse.clip(1e-7))
    return sim
