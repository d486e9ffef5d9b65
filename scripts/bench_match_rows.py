"""From a finished localisation to matches.csv: the per-box host loop against the match-rows stage.  Not bench.py: its timed
step ends at the box table and runs the same launches as before.

The planted synthetic set of bench.py (`--total-query-videos` query videos x 25 frames against 40 000 reference videos x 50
frames, 512-d, score-normalised, 20 % planted copies; 5 localised pairs per query video: 200 000 at the default size) goes
through `DeviceMatcher.match` once; then, from that result, in the same process:

  (a) the route of `vsc.baseline.sharded.match_sharded`: nbox / boxes / box_score copied to the host, compacted, one `Match`
      per box with two `get_timestamps` calls per side, then `Match.write_csv`;
  (b) the match-rows stage: the rows made on the device (`DeviceMatcher.match_rows`, what `match(rows=True)` adds to the
      step), `match_table` (one device-to-host copy per column), `MatchTable.write_csv`.

One JSON line per stage: wall time (perf_counter around the call; every stage returns synchronised; median, min and max
over --steps calls after --warmup for (b), over --host-steps calls for (a)) and, for the rows stage, the kernels' time
inside it (HIP events around the launches: vsc_aux_profile class 3).  `match()` and `match(rows=True)` are timed whole as
well (3 calls after 1 warm-up).  The last line holds the row counts, whether the two CSV files are byte-identical, the ratio (a) / (b) and the box.

    python scripts/bench_match_rows.py [--total-query-videos 40000] [--steps 7] [--warmup 2] [--host-steps 2]
"""
import argparse
import ctypes
import io
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--total-query-videos", type=int, default=40000)
    ap.add_argument("--query-frames", type=int, default=25)
    ap.add_argument("--ref-videos", type=int, default=40000)
    ap.add_argument("--ref-frames", type=int, default=50)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench  # the flagship workload's own input generators
    from vsc2022_amd import _lib
    from vsc2022_amd.engine import DeviceMatcher, DeviceScoreNormalizer
    from vsc2022_amd.vsc.index import VideoMetadata
    from vsc2022_amd.vsc.metrics import Match

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n_qv, qf, n_rv, rf, dim = args.total_query_videos, args.query_frames, args.ref_videos, args.ref_frames, args.dim
    refs = bench.synth_on_device(torch, dev, args.seed, n_rv, rf, dim, duplicates=True)
    queries = bench.synth_on_device(torch, dev, args.seed + 1000, n_qv, qf, dim)
    bench.plant_copies(torch, dev, args.seed + 2000, queries, n_qv, qf, refs, n_rv, rf)
    noise = bench.synth_on_device(torch, dev, args.seed + 77, n_rv * rf, 1, dim, static_frac=0.0)
    norm = DeviceScoreNormalizer(noise, beta=1.2)
    del noise
    q_off, r_off = np.arange(n_qv + 1, dtype=np.int64) * qf, np.arange(n_rv + 1, dtype=np.int64) * rf

    def stamps(n_vid, frames):  # half-second frames: [start, end] per frame, float32 as the feature files hold them
        t = np.tile(np.arange(frames, dtype=np.float32) * np.float32(0.5), n_vid)
        return np.stack([t, t + np.float32(0.5)], axis=1)

    q_ts, r_ts = stamps(n_qv, qf), stamps(n_rv, rf)
    q_ids, r_ids = [f"Q{k:06d}" for k in range(n_qv)], [f"R{k:06d}" for k in range(n_rv)]
    matcher = DeviceMatcher(norm.refs(refs), r_off, 0, r_ts=r_ts)
    matcher.set_queries(norm.queries(queries), q_off, q_ts=q_ts)
    del refs
    L = _lib.lib()
    _lib.check(L.vsc_aux_profile(1))

    def rows_kernel_ms():
        ms, cnt, by = ctypes.c_double(0.0), ctypes.c_int64(0), ctypes.c_double(0.0)
        _lib.check(L.vsc_aux_profile_read(3, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(by), 1))
        return ms.value, cnt.value

    def timed(label, fn, steps, warmup, kernels=False, **extra):
        for _ in range(warmup):
            fn()
        wall, kern, out = [], [], None
        for _ in range(steps):
            rows_kernel_ms()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(rows_kernel_ms())
        line = dict(stage=label, steps=steps, warmup=warmup, wall_ms_median=round(statistics.median(wall), 3),
                    wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3), **extra)
        if kernels:
            line["kernel_ms_median"] = round(statistics.median(k[0] for k in kern), 4)
            line["launch_groups_per_call"] = kern[-1][1]
        print(json.dumps(line), flush=True)
        return statistics.median(wall), out

    # (the whole step, for scale: seconds each, so fewer calls than the stages below)
    timed("match()", lambda: matcher.match(bias=0.5), 3, 1)
    timed("match(rows=True)", lambda: matcher.match(bias=0.5, rows=True), 3, 1, kernels=True)
    res = matcher.match(bias=0.5)
    n_loc = res.n_localized
    pq, pr = res.cand_q[:n_loc], res.cand_r[:n_loc]

    # ---- (a) the host route, as vsc/baseline/sharded.py:match_sharded runs it on the gathered box table
    q_meta = [VideoMetadata(video_id=q_ids[k], timestamps=q_ts[q_off[k]:q_off[k + 1]]) for k in range(n_qv)]
    r_meta = [VideoMetadata(video_id=r_ids[k], timestamps=r_ts[r_off[k]:r_off[k + 1]]) for k in range(n_rv)]

    def host_rows():
        cq, cr = res.cand_q.cpu().numpy(), res.cand_r.cpu().numpy()
        nbox, boxes, score = res.nbox.cpu().numpy(), res.boxes.cpu().numpy(), res.box_score.cpu().numpy()
        live = np.arange(_lib.TN_MAX_BOXES)[None, :] < nbox[:, None]
        cand = np.broadcast_to(res.loc_index.cpu().numpy()[:, None], live.shape)[live]
        table = np.concatenate([cand[:, None], boxes[live], score[live].view(np.int32)[:, None].astype(np.int64)], axis=1)
        matches = []
        for k, x1, y1, x2, y2, bits in table:
            q, r = q_meta[cq[k]], r_meta[cr[k]]
            s = np.array([bits], dtype=np.int64).astype(np.int32).view(np.float32)[0]
            matches.append(Match(query_id=q.video_id, ref_id=r.video_id, score=s,
                                 query_start=q.get_timestamps(int(x1))[0], query_end=q.get_timestamps(int(x2))[1],
                                 ref_start=r.get_timestamps(int(y1))[0], ref_end=r.get_timestamps(int(y2))[1]))
        return matches

    def csv_text(write, *a):
        buf = io.StringIO()
        write(*a, buf)
        return buf.getvalue()

    a_rows, matches = timed("(a) copy + compact + Match loop", host_rows, args.host_steps, 0)
    a_csv, text_a = timed("(a) Match.write_csv", lambda: csv_text(Match.write_csv, matches), args.host_steps, 0)

    # ---- (b) the match-rows stage
    def device_rows():
        return matcher._with_rows(res, pq, pr, res.n_matches, "maxsim")

    b_rows, _ = timed("(b) rows on the device", device_rows, args.steps, args.warmup, kernels=True, pairs=n_loc)
    b_table, table = timed("(b) match_table", lambda: matcher.match_table(res, q_ids, r_ids), args.steps, args.warmup)
    b_csv, text_b = timed("(b) MatchTable.write_csv", lambda: csv_text(table.write_csv), args.steps, args.warmup)
    a_ms, b_ms = a_rows + a_csv, b_rows + b_table + b_csv
    print(json.dumps({"pairs": n_loc, "rows_a": len(matches), "rows_b": len(table), "csv_bytes": len(text_a),
                      "csv_identical": text_a == text_b, "a_ms": round(a_ms, 1), "b_ms": round(b_ms, 1),
                      "a_over_b": round(a_ms / b_ms, 2), "a_over_b_without_csv": round(a_rows / (b_rows + b_table), 1),
                      "box": box()}), flush=True)


if __name__ == "__main__":
    main()
