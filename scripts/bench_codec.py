#!/usr/bin/env python3
"""Flat vs SQfp16 at BASELINE configs[1]'s shape: 200 k query x 2 M reference rows, 512-d, K = 1200 per query video
(what bench.py's config2_shape leg searches).  Both codecs are built on the SAME dec-rounded synthetic references, so
that both searches return the same hits and the figures compare storage, not data.

Per codec: ref_bytes, the time of `add` (device rows; fp32 for both, and half rows for SQfp16), the search's ms per
step (median and spread over --steps after --warmup, wall clock around a synchronised call) and the exact stage's ms
per step (kernel class 2 of vsc_index_profile_read_class, HIP events) beside the other kernel classes.  One JSON line per codec, then a summary line.

    python scripts/bench_codec.py [--steps 7] [--warmup 2] [--small]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a 20th of the shape (smoke run of the script)")
    args = ap.parse_args()

    import torch
    from bench import plant_copies, synth_on_device
    from vsc2022_amd import _lib
    from vsc2022_amd.vsc.index import FlatIndex

    dev = torch.device("cuda", 0)
    n_qv, qf, n_rv, rf, dim = (400, 25, 2000, 50, 512) if args.small else (8000, 25, 40000, 50, 512)
    refs = synth_on_device(torch, dev, 1, n_rv, rf, dim)
    queries = synth_on_device(torch, dev, 1001, n_qv, qf, dim)
    plant_copies(torch, dev, 2001, queries, n_qv, qf, refs, n_rv, rf)
    half = refs.to(torch.float16)
    refs = half.to(torch.float32)  # dec(refs): fp16-exact, what both codecs are built on
    K = 1200 * n_qv
    torch.cuda.synchronize()
    results, digest = {}, {}
    for codec in ("Flat", "SQfp16"):
        def build(rows):
            idx = FlatIndex(dim, _lib.METRIC_INNER_PRODUCT, 0, codec=codec)
            idx.use_torch_stream()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            idx.add(rows)
            torch.cuda.synchronize()
            return idx, (time.perf_counter() - t0) * 1e3

        idx, _ = build(refs)          # (first build: allocations + kernel loading)
        del idx
        idx, add_ms = build(refs)
        out = {"codec": codec, "rows": int(refs.shape[0]), "queries": int(queries.shape[0]), "dim": dim, "K": K,
               "add_fp32_ms": round(add_ms, 2)}
        if codec == "SQfp16":
            del idx
            idx, add16_ms = build(half)
            out["add_fp16_ms"] = round(add16_ms, 2)
        out["ref_bytes"] = int(idx.get_option("ref_bytes"))
        idx.profile(True)
        step_ms, exact_ms, classes = [], [], []
        for step in range(args.warmup + args.steps):
            idx.profile_read(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            i, j, s, radius = idx.global_topk(queries, K, device_out=True)
            torch.cuda.synchronize()
            if step >= args.warmup:
                step_ms.append((time.perf_counter() - t0) * 1e3)
                st = idx.profile_read(reset=True)
                exact_ms.append(st["rescore_ms"])
                classes.append(st)
        out.update(search_ms_per_step=round(statistics.median(step_ms), 2), search_ms_min=round(min(step_ms), 2),
                   search_ms_max=round(max(step_ms), 2), exact_stage_ms_per_step=round(statistics.median(exact_ms), 2),
                   exact_stage_ms_min=round(min(exact_ms), 2), exact_stage_ms_max=round(max(exact_ms), 2), hits=int(s.numel()),
                   radius=radius)
        # the other kernel classes of the handle's event timers (median per step): 0 the fp32 MFMA kernel of the dense first
        # batches, then the fp16 / int8 pre-filters, the int8 launches' preamble, re-threshold and final sort
        out["class_ms"] = {name: round(statistics.median(c[name + "_ms"] for c in classes), 2)
                           for name in ("sim", "f16", "i8", "i8_prep", "select", "sort")}
        digest[codec] = (int(i.long().sum().item()), int(j.long().sum().item()), int(s.view(torch.int32).long().sum().item()))
        results[codec] = out
        print(json.dumps(out), flush=True)
        del idx, i, j, s
        torch.cuda.empty_cache()
    a, b = results["SQfp16"], results["Flat"]
    print(json.dumps({"same_hits": digest["SQfp16"] == digest["Flat"], "ref_bytes_ratio": round(a["ref_bytes"] / b["ref_bytes"], 4),
                      "search_ratio": round(a["search_ms_per_step"] / b["search_ms_per_step"], 4),
                      "exact_stage_ratio": round(a["exact_stage_ms_per_step"] / max(b["exact_stage_ms_per_step"], 1e-9), 4)}))


if __name__ == "__main__":
    main()
