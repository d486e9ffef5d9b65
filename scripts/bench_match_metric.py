"""Scoring a finished matches table: the per-row host walk (`vsc.metrics.match_metric`) against the table route
(`match_metric_table` -> libvscmi's vsc_match_metric).  Not bench.py: its timed step ends at the box table.

Synthetic rows at the size of BASELINE configs[3]: `--pairs` (query, ref) pairs with 1-3 predictions each (about 2 x pairs
rows), ground truth of 1-2 segments on `--gt-pairs` of them; the first prediction of every ground-truth pair is a jittered
copy of its first segment with score + 0.5.  Scores and times are float32-born values held as float64.

One JSON line per stage: wall time (perf_counter around the stage; the entry point returns synchronised; median, min, max
over --steps calls after --warmup) -- `ordinals` (pair_ordinals: pandas.factorize), `upload` (the six arrays to HBM through
torch), `device` (vsc_match_metric on HBM-resident tables, whole call) with the kernels' time inside it split into `sorts`,
`pair_kernel` and `accumulate` (HIP events around the launches, reported in the call's stats block while
vsc_aux_profile is on; taken in separate calls), `tail`
(segment_ap_tail), and `table_route` (match_metric_table, everything from the two MatchTables).  `host` is
`match_metric(gt.to_matches(), pred.to_matches())`, the tuples built outside the timed region, over --host-steps calls.
The last line holds the counts, whether the two results agree bit for bit, the ratio host / table route and the box.

    python scripts/bench_match_metric.py [--pairs 200000] [--gt-pairs 5000] [--steps 5] [--warmup 1] [--host-steps 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def box():
    """The machine the numbers were taken on: GPU name, host CPU model."""
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(line.split(":", 1)[1].strip() for line in f if line.startswith("model name"))
    except (OSError, StopIteration):
        pass
    import torch

    return {"gpu": torch.cuda.get_device_name(0), "cpu": cpu}


def synthetic(n_pairs, n_gt_pairs, seed):
    """(gt, pred) MatchTables; five pairs per query video, one reference video per pair; prediction rows shuffled."""
    import numpy as np

    from vsc2022_amd.vsc.metrics import MatchTable

    rng = np.random.default_rng(seed)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)

    def boxes(n):
        lo = np.floor(rng.uniform(0.0, 40.0, (n, 2)) * 2) / 2
        hi = lo + 0.5 + np.floor(rng.uniform(0.0, 16.0, (n, 2)) * 2) / 2
        return np.stack([lo[:, 0], hi[:, 0], lo[:, 1], hi[:, 1]], axis=1)

    def as_table(pair, score, t):
        ids = MatchTable._ids
        q = np.char.add("Q", np.char.zfill((pair // 5).astype(str), 6))
        r = np.char.add("R", np.char.zfill(((pair * 7919) % 1000003).astype(str), 6))
        n = len(pair)
        return MatchTable(ids(q.tolist()), ids(r.tolist()), score, t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), t[:, 3].copy(),
                          np.full(n, -1, dtype=np.int64), np.full((n, 4), -1, dtype=np.int32))

    gt_of = rng.choice(n_pairs, n_gt_pairs, replace=False)
    gt_pair = np.repeat(gt_of, rng.integers(1, 3, n_gt_pairs))
    gt_t = boxes(len(gt_pair))
    pred_pair = np.repeat(np.arange(n_pairs), rng.integers(1, 4, n_pairs))
    pred_t = boxes(len(pred_pair))
    score = f32(rng.uniform(0.0, 1.0, len(pred_pair)))
    # the first prediction of every ground-truth pair: a jittered copy of its first segment, score + 0.5
    first_pred = np.flatnonzero(np.r_[True, pred_pair[1:] != pred_pair[:-1]])
    first_gt = {int(p): k for k, p in reversed(list(enumerate(gt_pair)))}
    for p in gt_of:
        k = first_pred[p]
        jitter = np.floor(rng.uniform(-1.0, 1.0, 4)) * 0.5 * np.array([1, -1, 1, -1])  # (starts earlier, ends later, or equal)
        pred_t[k] = gt_t[first_gt[int(p)]] + jitter
        score[k] = f32(np.array([score[k] + 0.5]))[0]
    shuffle = rng.permutation(len(pred_pair))
    return as_table(gt_pair, np.ones(len(gt_pair)), f32(gt_t)), as_table(pred_pair[shuffle], score[shuffle], f32(pred_t[shuffle]))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    walls, out = [], None
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, {"wall_ms": round(statistics.median(walls), 3), "min": round(min(walls), 3), "max": round(max(walls), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--gt-pairs", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import numpy as np
    import torch

    from vsc2022_amd import _lib
    from vsc2022_amd.vsc import metrics as M

    L = _lib.lib()
    gt, pred = synthetic(args.pairs, args.gt_pairs, args.seed)
    dev = torch.device("cuda", 0)

    def emit(stage, **kw):
        print(json.dumps({"stage": stage, **kw}), flush=True)

    (gt_pair, pred_pair, n_pairs, n_gt_pairs), t = timed(lambda: M.pair_ordinals(gt, pred), args.steps, args.warmup)
    emit("ordinals", **t)
    host_arrays = [gt_pair, M._times64(gt), pred_pair, np.ascontiguousarray(pred.score, dtype=np.float64), M._times64(pred)]

    def upload():
        out = [torch.from_numpy(a).to(dev) for a in host_arrays]
        torch.cuda.synchronize()
        return out

    on_dev, t = timed(upload, args.steps, args.warmup)
    emit("upload", bytes=int(sum(a.nbytes for a in host_arrays)), **t)

    def device_call():
        return M.device_group_sums(on_dev[0], on_dev[1], None, n_gt_pairs, on_dev[2], on_dev[3], on_dev[4], n_pairs, 0)

    device_call()
    (scores, sums, gt_len, stats), t = timed(device_call, args.steps, 0)
    _lib.check(L.vsc_aux_profile(1))  # (the events are kept out of the timed calls)
    try:
        profiled = [device_call()[3] for _ in range(args.steps)]
    finally:
        _lib.check(L.vsc_aux_profile(0))
    kernel = {name: round(statistics.median(int(p[4 + k]) for p in profiled) / 1e3, 3)
              for k, name in enumerate(("sorts", "pair_kernel", "accumulate"))}
    emit("device", kernel_ms=kernel, stats=[int(x) for x in stats[:4]], **t)
    res_tail, t = timed(lambda: M.segment_ap_tail(scores, sums, gt_len), args.steps, args.warmup)
    emit("tail", groups=int(len(scores)), **t)
    res_table, t_table = timed(lambda: M.match_metric_table(gt, pred), args.steps, args.warmup)
    emit("table_route", **t_table)

    gt_rows, pred_rows = gt.to_matches(), pred.to_matches()
    res_host, t_host = timed(lambda: M.match_metric(gt_rows, pred_rows), args.host_steps, 0)
    emit("host", **t_host)
    same = all(res_host.ap == r.ap and all(np.array_equal(getattr(res_host.pr_curve, f), getattr(r.pr_curve, f))
                                           for f in ("precisions", "recalls", "scores")) for r in (res_table, res_tail))
    emit("summary", pairs=int(n_pairs), gt_pairs=int(n_gt_pairs), pred_rows=len(pred), gt_rows=len(gt), groups=int(len(scores)),
         ap=res_host.ap, curve_points=int(len(res_host.pr_curve.scores)), bit_equal=bool(same),
         host_over_table=round(t_host["wall_ms"] / t_table["wall_ms"], 1), box=box())


if __name__ == "__main__":
    main()
