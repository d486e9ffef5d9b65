#!/usr/bin/env python3
"""Flat vs SQfp16 at BASELINE configs[1]'s shape: 200 k query x 2 M reference rows, 512-d, K = 1200 per query video
(what bench.py's config2_shape leg searches).  Both codecs are built on the SAME dec-rounded synthetic references, so
that both searches return the same hits and the figures compare storage, not data.

Per codec: ref_bytes, the time of `add` (device rows; fp32 for both, and half rows for SQfp16), the search's ms per
step (median and spread over --steps after --warmup, wall clock around a synchronised call) and the exact stage's ms
per step (kernel class 2 of vsc_index_profile_read_class, HIP events) beside the other kernel classes.  One JSON line per codec, then a summary line.

    python scripts/bench_codec.py [--steps 7] [--warmup 2] [--small]

`--leg tn`: the Temporal-Network context at BASELINE configs[3]'s shape -- 40000 query videos x 25 frames against 40000
reference videos x 50 frames (2 M rows), 513-d, `vsc_tn_localize` of the 200 k pairs of a step (5 per query video, the
planted copies among them, reference parameters, bias 0.5) -- with the references kept as fp32 (Flat) and as half floats
(SQfp16), in one process on the same dec-rounded rows.  The codecs alternate step by step.  Per codec: the bytes of the
reference rows (vsc_tn_ref_bytes), the time to create the context from device rows, ms per call (median and spread,
wall clock around the call, which returns synchronised) and the kernels' ms per call (HIP events, vsc_aux_profile class
1).  One JSON line per codec, then a summary line.  `--codecs Flat` times the Flat context alone, through vsc_tn_create:
the form that also runs on a library from before the codec, for a comparison on the same box.

    python scripts/bench_codec.py --leg tn [--steps 7] [--warmup 2] [--small] [--codecs Flat,SQfp16]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tn_leg(args):
    import numpy as np
    import torch
    from bench import plant_copies, synth_on_device
    from vsc2022_amd import _lib
    from vsc2022_amd.engine import REFERENCE_TN
    from vsc2022_amd.vcsl.vta import tn_params

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    n_qv, qf, n_rv, rf, dim = (2000, 25, 2000, 50, 513) if args.small else (40000, 25, 40000, 50, 513)
    refs = synth_on_device(torch, dev, 1, n_rv, rf, dim)
    queries = synth_on_device(torch, dev, 1001, n_qv, qf, dim)
    planted = plant_copies(torch, dev, 2001, queries, n_qv, qf, refs, n_rv, rf)
    half = refs.to(torch.float16).contiguous()
    refs = half.to(torch.float32).contiguous()  # dec(refs): both contexts see the same values
    per_q = 5
    g = torch.Generator(device="cpu")
    g.manual_seed(3001)
    pair_r = torch.randint(0, n_rv, (n_qv, per_q), generator=g, dtype=torch.int32)
    for qv, rv in planted:
        pair_r[qv, 0] = rv
    pair_q = torch.arange(n_qv, dtype=torch.int32).repeat_interleave(per_q).to(dev)
    pair_r = pair_r.reshape(-1).contiguous().to(dev)
    n = int(pair_q.numel())
    q_off = np.arange(n_qv + 1, dtype=np.int64) * qf
    r_off = np.arange(n_rv + 1, dtype=np.int64) * rf
    prm = tn_params(**REFERENCE_TN)
    nbox = torch.zeros(n, dtype=torch.int32, device=dev)
    boxes = torch.zeros((n, _lib.TN_MAX_BOXES, 4), dtype=torch.int32, device=dev)
    bmax = torch.zeros((n, _lib.TN_MAX_BOXES), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def create(codec, rows):
        ctx = ctypes.c_void_p()
        t0 = time.perf_counter()
        if codec == "Flat":
            _lib.check(L.vsc_tn_create(queries.data_ptr(), q_off.ctypes.data, n_qv, rows.data_ptr(), r_off.ctypes.data, n_rv, dim,
                                       _lib.MEM_DEVICE, 0, ctypes.byref(ctx)))
        else:
            _lib.check(L.vsc_tn_create_codec(queries.data_ptr(), q_off.ctypes.data, n_qv, rows.data_ptr(),
                                             int(rows.dtype == torch.float16), r_off.ctypes.data, n_rv, dim, _lib.MEM_DEVICE,
                                             _lib.MEM_DEVICE, _lib.CODECS[codec], 0, ctypes.byref(ctx)))
        return ctx, (time.perf_counter() - t0) * 1e3  # (the call returns with the rows in place)

    def aux_ms():
        ms, cnt, by = ctypes.c_double(0.0), ctypes.c_int64(0), ctypes.c_double(0.0)
        _lib.check(L.vsc_aux_profile_read(1, ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(by), 1))
        return ms.value

    def localize(ctx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(L.vsc_tn_localize(ctx, pair_q.data_ptr(), pair_r.data_ptr(), n, _lib.MEM_DEVICE, ctypes.byref(prm), 0.5,
                                     nbox.data_ptr(), boxes.data_ptr(), bmax.data_ptr(), _lib.MEM_DEVICE))
        return (time.perf_counter() - t0) * 1e3  # (the call returns synchronised)

    codecs = [c for c in args.codecs.split(",") if c]
    ctxs, out = {}, {}
    for codec in codecs:
        ctx, _ = create(codec, refs)  # (first create: allocations + kernel loading)
        L.vsc_tn_destroy(ctx)
        ctxs[codec], create_ms = create(codec, refs)
        out[codec] = {"leg": "tn", "codec": codec, "ref_rows": int(refs.shape[0]), "query_rows": int(queries.shape[0]), "dim": dim,
                      "pairs": n, "create_fp32_ms": round(create_ms, 2)}
        if codec == "SQfp16":
            L.vsc_tn_destroy(ctxs[codec])
            ctxs[codec], create16_ms = create(codec, half)
            out[codec]["create_fp16_ms"] = round(create16_ms, 2)
        if hasattr(L, "vsc_tn_ref_bytes"):
            out[codec]["ref_bytes"] = int(L.vsc_tn_ref_bytes(ctxs[codec]))
    _lib.check(L.vsc_aux_profile(1))
    wall = {c: [] for c in codecs}
    events = {c: [] for c in codecs}
    digest = {}
    for step in range(args.warmup + args.steps):
        for codec in codecs:  # (alternating: both codecs see the same state of the box)
            aux_ms()
            ms = localize(ctxs[codec])
            ev = aux_ms()
            if step >= args.warmup:
                wall[codec].append(ms)
                events[codec].append(ev)
            if step == args.warmup + args.steps - 1:
                valid = torch.arange(_lib.TN_MAX_BOXES, device=dev)[None, :] < nbox[:, None]
                digest[codec] = (int(nbox.long().sum().item()), int(boxes[valid].long().sum().item()),
                                 int(bmax[valid].view(torch.int32).long().sum().item()))
    for codec in codecs:
        out[codec].update(localize_ms=round(statistics.median(wall[codec]), 2), localize_ms_min=round(min(wall[codec]), 2),
                          localize_ms_max=round(max(wall[codec]), 2), kernel_ms=round(statistics.median(events[codec]), 2),
                          kernel_ms_min=round(min(events[codec]), 2), kernel_ms_max=round(max(events[codec]), 2),
                          boxes=digest[codec][0])
        print(json.dumps(out[codec]), flush=True)
        L.vsc_tn_destroy(ctxs[codec])
    if len(codecs) == 2:
        a, b = out["SQfp16"], out["Flat"]
        print(json.dumps({"same_boxes": digest["SQfp16"] == digest["Flat"], "ref_bytes_ratio": round(a["ref_bytes"] / b["ref_bytes"], 4),
                          "localize_ratio": round(a["localize_ms"] / b["localize_ms"], 4),
                          "kernel_ratio": round(a["kernel_ms"] / b["kernel_ms"], 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a 20th of the shape (smoke run of the script)")
    ap.add_argument("--leg", choices=("index", "tn"), default="index")
    ap.add_argument("--codecs", default="Flat,SQfp16", help="--leg tn: the contexts to time")
    args = ap.parse_args()
    if args.leg == "tn":
        return tn_leg(args)

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
