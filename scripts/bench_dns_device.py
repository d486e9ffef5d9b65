"""The DnS baseline's localisation: the reference's per-pair host route against `VCSLLocalizationDnS(on_device=True)`.
Not bench.py: the flagship workload is the SSCD baseline.

Synthetic data of the project's own (vsc2022_amd.synth): 60-frame videos, 512-d coarse descriptors, fine descriptors
derived from them as tests/helpers.py:g9_inputs does (R = 9 regions x D = 512, unit rows), a fifth of the queries
holding a planted copy; every query video is paired with --per-query references, the reference's parameters
(TN, tn_max_step 5, min_length 4, bias 0.5, symmetric, geometric mean), batches of 512 pairs as localize_and_verify runs
them.  Three routes through `localize_all`:

  host            on_device=False with ChamferSimilarity on "cuda": two uploads, two model calls, a .cpu(), one
                  vsc_tn_similarity and its copy per pair, numpy blend, one vsc_tn_forward_sim upload per batch
  device/chamfer  on_device=True, ChamferSimilarity in libvscmi (vsc_tn_fine_similarity + vsc_tn_localize_fine)
  device/torch    on_device=True, the same module scripted (any torch model's route: per pair on the GPU into one slab)

Per route one JSON line: wall time (perf_counter; the calls return synchronised) and device time (torch.cuda events on
the stream the work runs on) of all batches, median and spread over --steps runs after --warmup; stage 1 of the
chamfer route alone with its TFLOP/s (2 Lq Lr R^2 D flops per pair); the matches of the three routes compared; the box.

--fine_codec bits adds the binary student's leg: the same videos with binary fine descriptors (the sign of the
projections, as dns_index writes `feature > 0`) through `ChamferSimilarity("bin")` on the device, once with the default
+-1 fp32 store and once with the 1-bit store.  Stage 1 of both is timed in ALTERNATING repetitions in the same process
(--stage-reps passes over all batches per timing, so that a window is not a fraction of a millisecond of launches);
one JSON line holds both stores' times and `fine_bytes`, their ratio, and whether the two slabs and the two routes'
matches are equal bit for bit.  --skip-routes leaves the three att routes out.

--fine_codec SQfp16 adds the attention student's leg in the same way: the same videos with the fine descriptors cast to
float16 (what dns_index writes for an attention student) through `ChamferSimilarity("att")` on the device, once with the
default fp32 store and once with the half-float store.  Besides the above the line holds the fp32 store's own spread,
(max - min) / median of its stage-1 device times, and whether the half store's median stays within it.

    python scripts/bench_dns_device.py [--queries 256] [--per-query 8] [--steps 5] [--warmup 1] [--host-steps 2]
                                       [--fine_codec bits|SQfp16] [--stage-reps 10] [--skip-routes]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def box():
    import torch

    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next((line.split(":", 1)[1].strip() for line in f if line.startswith("model name")), cpu)
    except OSError:
        pass
    return {"gpu": torch.cuda.get_device_name(0), "cpu": cpu, "host": os.uname().nodename, "torch": torch.__version__}


def make_inputs(np, n_query, per_query, regions, fdim, frames=60, dim=512, seed=5, binary=False):
    from vsc2022_amd import synth
    from vsc2022_amd.vsc.index import VideoFeature
    from vsc2022_amd.vsc.metrics import CandidatePair

    q, r, gts = synth.make_dataset(seed=seed, n_query=n_query, n_ref=n_query, dim=dim, q_frames=(frames, frames),
                                 r_frames=(frames, frames), planted_frac=0.2, noise=0.03)
    qc, rc = synth.to_video_features(q, VideoFeature), synth.to_video_features(r, VideoFeature)
    rng = np.random.default_rng(seed + 1)
    proj = rng.standard_normal((regions, dim, fdim)).astype(np.float32)

    def fine(v):
        x = np.einsum("ld,rde->lre", np.asarray(v.feature, dtype=np.float32), proj)
        x += 0.05 * rng.standard_normal(x.shape).astype(np.float32)
        if binary:
            return VideoFeature(video_id=v.video_id, timestamps=v.timestamps, feature=x > 0)
        return VideoFeature(video_id=v.video_id, timestamps=v.timestamps,
                            feature=(x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32))

    qf, rf = [fine(v) for v in qc], [fine(v) for v in rc]
    copied = {g.query_id: g.ref_id for g in gts}  # a planted copy's reference comes first among the query's pairs
    r_ord = {v.video_id: n for n, v in enumerate(rc)}
    cands = []
    for k, v in enumerate(qc):
        first = r_ord[copied[v.video_id]] if v.video_id in copied else k
        cands += [CandidatePair(v.video_id, rc[(first + 37 * j) % len(rc)].video_id, 1.0 - 1e-4 * j) for j in range(per_query)]
    return qc, rc, qf, rf, cands


def timed(torch, fn, steps, warmup):
    wall, dev, out = [], [], None
    for step in range(warmup + steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if step >= warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(a.elapsed_time(b))
    return {"wall": stat(wall), "device": stat(dev)}, out


def stat(x):
    return {"median_ms": round(statistics.median(x), 3), "min_ms": round(min(x), 3), "max_ms": round(max(x), 3), "runs": len(x)}


def fine_codec_leg(np, torch, args, kw):
    """A student on the device, the default fp32 store against `--fine_codec`'s store, stage 1 in alternating repetitions:
    the binary student (+-1 fp32 against bits) or the attention student on float16 descriptors (fp32 against halves)."""
    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity, VCSLLocalizationDnS
    from vsc2022_amd.vsc.index import VideoFeature

    binary = args.fine_codec == "bits"
    plain, coded = ("bin_fp32", "bits") if binary else ("att_fp32", "att_f16")
    qc, rc, qf, rf, cands = make_inputs(np, args.queries, args.per_query, args.regions, args.fdim, binary=binary)
    if not binary:
        qf, rf = ([VideoFeature(video_id=v.video_id, timestamps=v.timestamps, feature=v.feature.astype(np.float16)) for v in side]
                  for side in (qf, rf))
    model = ChamferSimilarity("bin" if binary else "att")
    locs = {plain: VCSLLocalizationDnS(model, qf, rf, qc, rc, on_device=True, **kw),
            coded: VCSLLocalizationDnS(model, qf, rf, qc, rc, on_device=True, fine_codec=args.fine_codec, **kw)}
    parts = [cands[start:start + 512] for start in range(0, len(cands), 512)]
    flops = 2.0 * sum(len(locs[coded].queries[c.query_id]) * len(locs[coded].refs[c.ref_id]) for c in cands) * args.regions ** 2 * args.fdim

    def stage1(loc, keep=False):
        slabs = []
        for part in parts:
            slab, _ = loc._fine_slab(part, *loc._pair_ordinals(part))
            if keep:
                slabs.append(slab)
        return slabs

    torch.cuda.synchronize()
    slabs = {name: [s.cpu().numpy().view(np.uint32) for s in stage1(loc, keep=True)] for name, loc in locs.items()}
    same_slabs = all(np.array_equal(a, b) for a, b in zip(slabs[plain], slabs[coded]))
    wall, dev = {n: [] for n in locs}, {n: [] for n in locs}
    for step in range(args.warmup + args.steps):
        for name, loc in locs.items():  # alternating: a drift of the box lands on both
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.stage_reps):
                stage1(loc)
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if step >= args.warmup:
                wall[name].append((t1 - t0) * 1e3 / args.stage_reps)
                dev[name].append(a.elapsed_time(b) / args.stage_reps)
    student = "binary" if binary else "attention"
    out = {"stage": "vsc_tn_fine_similarity, %s student" % student, "pairs": len(cands), "batches": len(parts), "regions": args.regions,
           "fdim": args.fdim, "stage_reps": args.stage_reps, "g_bit_products" if binary else "g_products": round(flops / 2e9, 2),
           "slabs_equal_bitwise": same_slabs}
    for name, loc in locs.items():
        out[name] = {"wall": stat(wall[name]), "device": stat(dev[name]), "fine_bytes": loc.fine_bytes,
                     "tera_products_per_s_device_median": round(flops / 2 / (statistics.median(dev[name]) * 1e-3) / 1e12, 2)}
    tag = "bits" if binary else "f16"
    out["device_time_ratio_fp32_over_" + tag] = round(out[plain]["device"]["median_ms"] / out[coded]["device"]["median_ms"], 2)
    out["fine_bytes_ratio_fp32_over_" + tag] = round(out[plain]["fine_bytes"] / out[coded]["fine_bytes"], 2)
    if not binary:  # the half store buys bytes, not time: its median must stay within the fp32 store's own spread
        spread = (max(dev[plain]) - min(dev[plain])) / statistics.median(dev[plain])
        out["fp32_device_spread"] = round(spread, 4)
        out["fine_bytes_exactly_half"] = out[coded]["fine_bytes"] * 2 == out[plain]["fine_bytes"]
        out["f16_not_slower"] = statistics.median(dev[coded]) <= statistics.median(dev[plain]) * (1.0 + spread)
    print(json.dumps(out), flush=True)

    def batches(loc):
        found = []
        for part in parts:
            found += loc.localize_all(part)
        return found

    res, found = {}, {}
    for name, loc in locs.items():
        res[name], found[name] = timed(torch, lambda: batches(loc), args.steps, args.warmup)
    same = len(found[coded]) == len(found[plain]) and all(
        a._replace(score=0.0) == b._replace(score=0.0) and np.float32(a.score).view(np.uint32) == np.float32(b.score).view(np.uint32)
        for a, b in zip(found[coded], found[plain]))
    print(json.dumps({"route": "device/chamfer, %s student, both stages" % student, "matches": len(found[coded]),
                      "matches_equal_bitwise": same, **{name: res[name] for name in locs}, "box": box()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--per-query", type=int, default=8)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--fdim", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--fine_codec", choices=["bits", "SQfp16"], default=None)
    ap.add_argument("--stage-reps", type=int, default=10)
    ap.add_argument("--skip-routes", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from vsc2022_amd.vsc.baseline.dns_baseline import ChamferSimilarity, VCSLLocalizationDnS

    kw = dict(model_type="TN", tn_max_step=5, min_length=4, concurrency=16, similarity_bias=0.5, device="cuda")
    if args.fine_codec:
        fine_codec_leg(np, torch, args, kw)
    if args.skip_routes:
        return
    qc, rc, qf, rf, cands = make_inputs(np, args.queries, args.per_query, args.regions, args.fdim)
    model = ChamferSimilarity("att")
    routes = {
        "host": (VCSLLocalizationDnS(model, qf, rf, qc, rc, **kw), args.host_steps, min(args.warmup, 1)),
        "device/chamfer": (VCSLLocalizationDnS(model, qf, rf, qc, rc, on_device=True, **kw), args.steps, args.warmup),
        "device/torch": (VCSLLocalizationDnS(torch.jit.script(ChamferSimilarity("att")).to("cuda"), qf, rf, qc, rc,
                                             on_device=True, **kw), args.steps, args.warmup),
    }

    def batches(loc):
        found = []
        for start in range(0, len(cands), 512):
            found += loc.localize_all(cands[start:start + 512])
        return found

    results, matches = {}, {}
    for name, (loc, steps, warmup) in routes.items():
        results[name], matches[name] = timed(torch, lambda: batches(loc), steps, warmup)
        print(json.dumps({"route": name, "pairs": len(cands), "matches": len(matches[name]), **results[name]}), flush=True)

    # stage 1 of the chamfer route alone, in batches of 512 pairs
    loc = routes["device/chamfer"][0]
    flops = 2.0 * sum(len(loc.queries[c.query_id]) * len(loc.refs[c.ref_id]) for c in cands) * args.regions ** 2 * args.fdim

    def stage1():
        for start in range(0, len(cands), 512):
            part = cands[start:start + 512]
            loc._fine_slab(part, *loc._pair_ordinals(part))

    s1, _ = timed(torch, stage1, args.steps, args.warmup)
    print(json.dumps({"stage": "vsc_tn_fine_similarity", "gflop": round(flops / 1e9, 2), **s1,
                      "tflops_device_median": round(flops / (s1["device"]["median_ms"] * 1e-3) / 1e12, 2),
                      "fine_bytes": loc.fine_bytes}), flush=True)

    key = lambda m: (m.query_id, m.ref_id, float(m.query_start), float(m.query_end), float(m.ref_start), float(m.ref_end))
    same_boxes = {n: [key(m) for m in matches[n]] == [key(m) for m in matches["host"]] for n in matches}
    worst = {n: max((abs(float(a.score) - float(b.score)) for a, b in zip(matches[n], matches["host"])), default=0.0)
             if same_boxes[n] else None for n in matches}
    host = results["host"]["wall"]["median_ms"]
    print(json.dumps({"same_boxes_as_host": same_boxes, "max_score_difference_to_host": worst,
                      "torch_route_equal_to_host": matches["device/torch"] == matches["host"],
                      "wall_ratio_host_over": {n: round(host / results[n]["wall"]["median_ms"], 2) for n in results},
                      "box": box()}), flush=True)


if __name__ == "__main__":
    main()
