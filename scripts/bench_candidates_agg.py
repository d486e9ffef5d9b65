"""Candidate tables by max / sum / mean / top-m mean on the device (vsc_pair_aggregate, csrc/pair_reduce.hip) against the
generic host route (VideoIndex.search's regroup -> one aggregate() per pair -> sorted).  Not bench.py: its step calls
vsc_pair_max as before.

The hit lists are synthetic, generated in HBM from a seed (no search is timed here): every hit is a (query row, ref row,
score) triple, half of them between a query video and one of its --planted favoured reference videos (so that pairs hold
many hits, as copies do), the rest spread uniformly; scores uniform in [0, 1).

  knn        BASELINE configs[1]'s shape: 200 000 query rows x k = --knn-k neighbours over 2 000 000 reference rows
             (8 000 query videos x 25 frames, 40 000 reference videos x 50 frames);
  desc       the descriptor track's constants: 40 000 query videos x 1 200 hits = 48 M hits over 1 000 000 query rows and
             2 000 000 reference rows.

Each list is timed in both orders -- search order (score descending; hits_order = 1) and (row, rank) order (rows
ascending, scores descending inside a row; hits_order = 0) -- for max, sum, mean and topmean(--top-m); on the search-order
list vsc_pair_max is timed beside VSC_AGG_MAX.  Wall time per call (perf_counter around a call that returns synchronised;
median, min, max over --steps calls after --warmup).  The generic route runs on the same generator at --generic-videos
query videos (default 2 000: 2.4 M hits -- the size at which it finishes in about a minute per aggregation), together
with the device route on that very list, and the two tables are compared (ids and score bits).

    python scripts/bench_candidates_agg.py [--steps 5] [--warmup 2] [--skip-desc] [--generic-videos 2000]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hit_list(torch, dev, seed, n_qvid, q_frames, n_rvid, r_frames, n_hits, planted, per_row=None):
    """(i, j, s) int32 / int32 / fp32 in HBM, unordered.  per_row: exactly that many hits for every query row (a k-NN
    result), else rows drawn uniformly."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nq_rows = n_qvid * q_frames
    if per_row:
        i = torch.arange(nq_rows, device=dev, dtype=torch.int64).repeat_interleave(per_row)
    else:
        i = torch.randint(0, nq_rows, (n_hits,), device=dev, generator=g)
    n = int(i.numel())
    qv = i // q_frames
    fav = (qv * 7919 + torch.randint(0, planted, (n,), device=dev, generator=g) * 104729) % n_rvid
    rv = torch.where(torch.rand(n, device=dev, generator=g) < 0.5, fav, torch.randint(0, n_rvid, (n,), device=dev, generator=g))
    j = rv * r_frames + torch.randint(0, r_frames, (n,), device=dev, generator=g)
    s = torch.rand(n, device=dev, generator=g)
    return i.to(torch.int32), j.to(torch.int32), s


def search_order(torch, i, j, s):
    o = torch.argsort(s, descending=True, stable=True)
    return i[o].contiguous(), j[o].contiguous(), s[o].contiguous()


def row_rank_order(torch, i, j, s):
    o = torch.argsort(s, descending=True, stable=True)
    o = o[torch.argsort(i[o].to(torch.int64), stable=True)]
    return i[o].contiguous(), j[o].contiguous(), s[o].contiguous()


class Aggregator:
    """vsc_pair_aggregate / vsc_pair_max on device arrays, with preallocated outputs."""

    def __init__(self, torch, dev, row2q, row2r, cap):
        self.torch, self.dev, self.row2q, self.row2r = torch, dev, row2q, row2r
        self.out = [torch.empty(cap, dtype=d, device=dev) for d in (torch.int32, torch.int32, torch.float32, torch.int64, torch.int32)]

    def __call__(self, i, j, s, agg, top_m, hits_order, pair_max=False):
        import ctypes

        from vsc2022_amd import _lib

        n = int(s.numel())
        n_pairs = ctypes.c_int64(0)
        o = [t.data_ptr() for t in self.out]
        self.torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        if pair_max:
            _lib.check(_lib.lib().vsc_pair_max(i.data_ptr(), j.data_ptr(), s.data_ptr(), n, _lib.MEM_DEVICE, self.row2q.data_ptr(),
                                               int(self.row2q.numel()), self.row2r.data_ptr(), int(self.row2r.numel()), _lib.MEM_DEVICE,
                                               o[0], o[1], o[2], o[3], n, _lib.MEM_DEVICE, ctypes.byref(n_pairs), self.dev.index))
        else:
            _lib.check(_lib.lib().vsc_pair_aggregate(i.data_ptr(), j.data_ptr(), s.data_ptr(), n, _lib.MEM_DEVICE, self.row2q.data_ptr(),
                                                     int(self.row2q.numel()), self.row2r.data_ptr(), int(self.row2r.numel()),
                                                     _lib.MEM_DEVICE, hits_order, agg, top_m, o[0], o[1], o[2], o[3], o[4], n,
                                                     _lib.MEM_DEVICE, ctypes.byref(n_pairs), self.dev.index))
        return time.perf_counter() - t0, n_pairs.value


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts, last = [], None
    for _ in range(steps):
        t, last = fn()
        ts.append(t * 1e3)
    return {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "pairs": last}


def generic_route(np, i, j, s, row2q, row2r, n_qvid, n_rvid, aggregation):
    """CandidateGeneration.query's generic route on a given hit list: VideoIndex.search (regroup + PairMatches) with the
    search itself replaced by the list, then aggregation.score per pair and sorted -- the code of vsc/index.py and
    vsc/candidates.py, unchanged."""
    from vsc2022_amd.vsc.index import SearchHits, VideoIndex, VideoMetadata

    meta = VideoMetadata("v", np.zeros(1, dtype=np.float32))
    index = VideoIndex.__new__(VideoIndex)
    index._video_ids = list(range(n_rvid))
    index._row2vid = row2r
    index._row2frame = np.zeros(len(row2r), dtype=np.int32)
    index.video_metadata = {k: meta for k in range(n_rvid)}
    layout = types.SimpleNamespace(video_ids=list(range(n_qvid)), row2vid=row2q, row2frame=np.zeros(len(row2q), dtype=np.int32),
                                   metadata=[meta] * n_qvid)
    index.search_hits = lambda queries, global_k: SearchHits(i, j, s, layout, index)
    t0 = time.perf_counter()
    matches = index.search(None, 1)
    t1 = time.perf_counter()
    candidates = [aggregation.score(match) for match in matches]
    t2 = time.perf_counter()
    candidates = sorted(candidates, key=lambda match: match.score, reverse=True)
    t3 = time.perf_counter()
    return candidates, {"regroup_s": round(t1 - t0, 3), "aggregate_s": round(t2 - t1, 3), "sort_s": round(t3 - t2, 3),
                        "total_s": round(t3 - t0, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--knn-k", type=int, default=10)
    ap.add_argument("--top-m", type=int, default=5)
    ap.add_argument("--planted", type=int, default=3)
    ap.add_argument("--generic-videos", type=int, default=2000)
    ap.add_argument("--skip-desc", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import numpy as np
    import torch

    from vsc2022_amd import _lib
    from vsc2022_amd.vsc import candidates as C

    if not torch.cuda.is_available() or _lib.device_count() <= 0:
        raise SystemExit("bench_candidates_agg: no gfx950 device (there is no CPU fallback)")
    dev = torch.device("cuda", 0)
    q_frames, n_rvid, r_frames = 25, 40000, 50
    row2r = torch.arange(n_rvid, device=dev, dtype=torch.int32).repeat_interleave(r_frames)
    modes = [("max", _lib.AGG_MAX, 1), ("sum", _lib.AGG_SUM, 1), ("mean", _lib.AGG_MEAN, 1), (f"topmean{args.top_m}", _lib.AGG_TOPMEAN, args.top_m)]
    shapes = [("knn", 8000, None, args.knn_k)]
    if not args.skip_desc:
        shapes.append(("desc", 40000, 1200 * 40000, None))
    for shape, n_qvid, n_hits, per_row in shapes:
        row2q = torch.arange(n_qvid, device=dev, dtype=torch.int32).repeat_interleave(q_frames)
        raw = hit_list(torch, dev, args.seed, n_qvid, q_frames, n_rvid, r_frames, n_hits, args.planted, per_row)
        run = Aggregator(torch, dev, row2q, row2r, int(raw[2].numel()))
        for order_name, hits_order, make in (("search", 1, search_order), ("row_rank", 0, row_rank_order)):
            i, j, s = make(torch, *raw)
            for name, agg, m in modes:
                res = timed(lambda: run(i, j, s, agg, m, hits_order), args.steps, args.warmup)
                print(json.dumps({"stage": "device", "shape": shape, "order": order_name, "agg": name, "hits": int(s.numel()), **res}), flush=True)
            if hits_order:
                res = timed(lambda: run(i, j, s, 0, 1, 1, pair_max=True), args.steps, args.warmup)
                print(json.dumps({"stage": "device", "shape": shape, "order": order_name, "agg": "vsc_pair_max", "hits": int(s.numel()), **res}),
                      flush=True)
            del i, j, s
        del raw, run
        torch.cuda.empty_cache()

    # ---- the generic route, and the device route on the same list
    n_qvid = args.generic_videos
    row2q = torch.arange(n_qvid, device=dev, dtype=torch.int32).repeat_interleave(q_frames)
    i, j, s = search_order(torch, *hit_list(torch, dev, args.seed + 1, n_qvid, q_frames, n_rvid, r_frames, 1200 * n_qvid, args.planted))
    run = Aggregator(torch, dev, row2q, row2r, int(s.numel()))
    hi, hj, hs = i.cpu().numpy(), j.cpu().numpy(), s.cpu().numpy()
    hq, hr = row2q.cpu().numpy(), row2r.cpu().numpy()
    for name, agg, m in modes:
        dres = timed(lambda: run(i, j, s, agg, m, 1), args.steps, args.warmup)
        k = dres["pairs"]
        dq, dr, ds = (t[:k].cpu().numpy() for t in run.out[:3])
        aggregation = {"max": C.MaxScoreAggregation, "sum": C.SumScoreAggregation, "mean": C.MeanScoreAggregation}.get(name)
        aggregation = aggregation() if aggregation else C.TopMeanScoreAggregation(m)
        cands, gres = generic_route(np, hi, hj, hs, hq, hr, n_qvid, n_rvid, aggregation)
        same = (len(cands) == k and np.array_equal([c.query_id for c in cands], dq) and np.array_equal([c.ref_id for c in cands], dr)
                and np.array_equal(np.array([c.score for c in cands], dtype=np.float32).view(np.uint32), ds.view(np.uint32)))
        print(json.dumps({"stage": "generic_vs_device", "query_videos": n_qvid, "hits": int(s.numel()), "agg": name, "pairs": k,
                          "device_ms_median": dres["ms_median"], **gres, "tables_equal": bool(same),
                          "ratio": round(gres["total_s"] * 1e3 / dres["ms_median"], 1)}), flush=True)
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(line.split(":", 1)[1].strip() for line in f if line.startswith("model name"))
    except (OSError, StopIteration):
        pass
    print(json.dumps({"stage": "box", "gpu": torch.cuda.get_device_name(0), "cpu": cpu, "steps": args.steps, "warmup": args.warmup}), flush=True)


if __name__ == "__main__":
    main()
