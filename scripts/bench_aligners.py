"""DTW / DP on the host against DTW / DP on the GPU (`on_device=True`), with the Temporal Network's fused route beside
them for scale.  Not bench.py: the flagship workload never asks for these aligners.

N candidate pairs of BASELINE configs[1]-like videos (25 query frames, 50 reference frames, 512-d unit rows; a fifth of
the query videos carry a noised copy of a reference segment and are paired with that reference first), aligned through
`VCSLLocalizationMaxSim(queries, refs, name, ...).localize_all(candidates)`:

  host    the reference's route: one vsc_tn_similarity call and one device-to-host copy per pair, the aligner in Python
  device  `on_device=True`: one vsc_tn_align call for the batch
  TN      the fused Temporal-Network route (vsc_tn_localize), the reference's parameters

Per route one JSON line: wall time of `localize_all` (perf_counter around the call, which returns synchronised; median
and spread over --steps calls after --warmup; the host routes run --host-steps calls) and the kernels' time inside it
(HIP events around the launches: vsc_aux_profile class 2 for DTW / DP, class 1 for TN).  The device routes' matches are
compared with the host routes' (ids, timestamps, score bits); a last line holds the wall-time ratios and the box.

    python scripts/bench_aligners.py [--pairs 4096] [--steps 7] [--warmup 2] [--host-steps 1]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_set(np, n_pairs, qf, rf, dim, per_q=4, frac=0.2, noise=0.05, seed=1):
    from vsc2022_amd.vsc.index import VideoFeature
    from vsc2022_amd.vsc.metrics import CandidatePair

    rng = np.random.default_rng(seed)
    n_q = (n_pairs + per_q - 1) // per_q
    n_r = n_q

    def videos(n, frames, prefix):
        x = rng.standard_normal((n, frames, dim)).astype(np.float32)
        x /= np.linalg.norm(x, axis=2, keepdims=True)
        ts = np.stack([np.arange(frames, dtype=np.float32), np.arange(1, frames + 1, dtype=np.float32)], axis=1)
        return [VideoFeature(video_id=f"{prefix}{v:06d}", timestamps=ts, feature=x[v]) for v in range(n)]

    queries, refs = videos(n_q, qf, "Q"), videos(n_r, rf, "R")
    pair_r = rng.integers(0, n_r, (n_q, per_q))
    length = min(qf, rf) * 3 // 5
    for qv in rng.permutation(n_q)[: int(round(frac * n_q))]:
        rv = int(pair_r[qv, 0])
        q0, r0 = int(rng.integers(0, qf - length + 1)), int(rng.integers(0, rf - length + 1))
        seg = refs[rv].feature[r0 : r0 + length] + noise * rng.standard_normal((length, dim)).astype(np.float32)
        queries[qv].feature[q0 : q0 + length] = seg / np.linalg.norm(seg, axis=1, keepdims=True)
    cands = [CandidatePair(queries[qv].video_id, refs[int(pair_r[qv, k])].video_id, 1.0) for qv in range(n_q) for k in range(per_q)]
    return queries, refs, cands[:n_pairs]


def box():
    """The machine the numbers were taken on: GPU name, host CPU model."""
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(line.split(":", 1)[1].strip() for line in f if line.startswith("model name"))
    except (OSError, StopIteration):
        pass
    try:
        import torch

        gpu = torch.cuda.get_device_name(0)
    except Exception:
        gpu = "unknown"
    return {"gpu": gpu, "cpu": cpu}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--query-frames", type=int, default=25)
    ap.add_argument("--ref-frames", type=int, default=50)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-steps", type=int, default=1)
    args = ap.parse_args()

    import numpy as np
    from vsc2022_amd import _lib
    from vsc2022_amd.engine import REFERENCE_TN
    from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim

    L = _lib.lib()
    queries, refs, cands = make_set(np, args.pairs, args.query_frames, args.ref_frames, args.dim)
    _lib.check(L.vsc_aux_profile(1))

    def aux_ms(cls):
        ms, cnt, by = ctypes.c_double(0.0), ctypes.c_int64(0), ctypes.c_double(0.0)
        _lib.check(L.vsc_aux_profile_read(cls, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(by), 1))
        return ms.value

    def run(label, loc, steps, warmup, cls):
        for _ in range(warmup):
            loc.localize_all(cands)
        wall, kern, out = [], [], None
        for _ in range(steps):
            aux_ms(cls)
            t0 = time.perf_counter()
            out = loc.localize_all(cands)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(aux_ms(cls))
        line = {"route": label, "pairs": len(cands), "matches": len(out), "steps": steps, "warmup": warmup,
                "wall_ms_median": round(statistics.median(wall), 3), "wall_ms_min": round(min(wall), 3),
                "wall_ms_max": round(max(wall), 3)}
        if cls is not None and any(kern):
            line["kernel_ms_median"] = round(statistics.median(kern), 3)
        print(json.dumps(line), flush=True)
        return statistics.median(wall), out

    def same(a, b):
        return len(a) == len(b) and all(
            x[:2] == y[:2] and x[3:] == y[3:] and np.float32(x.score).view(np.uint32) == np.float32(y.score).view(np.uint32)
            for x, y in zip(a, b))

    kw = dict(min_sim=0.5, min_length=4)
    ratios = {"pairs": len(cands), "frames": [args.query_frames, args.ref_frames], "dim": args.dim}
    for name in ("DTW", "DP"):
        host_ms, host_out = run(f"{name} host", VCSLLocalizationMaxSim(queries, refs, name, **kw), args.host_steps, 0, 2)
        dev_ms, dev_out = run(f"{name} device", VCSLLocalizationMaxSim(queries, refs, name, on_device=True, **kw), args.steps,
                              args.warmup, 2)
        ratios[f"{name}_host_over_device_wall"] = round(host_ms / dev_ms, 1)
        ratios[f"{name}_identical"] = same(host_out, dev_out)
    run("TN fused", VCSLLocalizationMaxSim(queries, refs, "TN", **REFERENCE_TN), args.steps, args.warmup, 1)
    ratios["box"] = box()
    print(json.dumps(ratios), flush=True)


if __name__ == "__main__":
    main()
