#!/usr/bin/env python3
"""DnS L3-iMAC region descriptors ([frames, 9, 3840]) on synthetic 224 x 224 videos, one GPU: 25 frames per video, packed
batches of 128 (the batch size of the reference's DnS command).  Three legs on the same seeded videos:

  fp32-eager     fp32 `L3iMACModel`, one video per batch (what the reference runs through TorchScript)
  bf16-autocast  the BatchNorm-folded network under bf16 autocast, channels-last, packed batches
  FastL3iMAC     the library's kernels (inference_l3imac.FastL3iMAC), packed batches

fp32-eager runs once; the two fast legs alternate for --rounds rounds so that the run-to-run spread is seen.  Then the
region stage alone (four pools + the row normalisation of one batch, on the bf16 taps of a real forward pass) is timed
with device events against the same stage written as torch ops on those taps, and its algorithmic bytes are printed:
2 B sum_t H_t W_t C_t (the bf16 taps, read once) + 4 B R 3840 (the fp32 rows, written once).

--legs picks a subset; `--legs FastL3iMAC --stage-only` is the program for a `rocprofv3 --kernel-trace --stats` run."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from vsc2022_amd.vsc.baseline import inference_l3imac as il
from vsc2022_amd.vsc.baseline.inference import SyntheticVideos, fold_batchnorm, preprocess, run_inference, run_inference_packed, \
    to_flat

HBM_COPY_RATE = 6.29e12  # measured copy rate of one MI355X, bytes/s (profiles/r02_roofline.json)


def stage_bytes(batch: int, size: int) -> int:
    """Algorithmic bytes of the region stage for `batch` frames of size x size: every bf16 tap element read once, every
    fp32 output element written once."""
    def half(n):  # a stride-2 convolution or pool with "same" padding
        return (n - 1) // 2 + 1

    taps, side = 0, half(half(size))  # the stem halves twice; every later stage once
    for i, c in enumerate(il.TAP_CHANNELS):
        side = side if i == 0 else half(side)
        taps += side * side * c
    gh, gw = il._grid(side, side, il.TAP_WINDOWS[-1], il.TAP_STRIDES[-1])
    return 2 * batch * taps + 4 * batch * gh * gw * il.L3IMAC_DIMS


def torch_stage(taps):
    """The region stage as torch ops on the bf16 taps (what FastL3iMAC would run without csrc/region_pool.hip), at its
    leanest: the pool on the bf16 NHWC tensor (exact), fp32 from there, and like `fast_stage` without the adaptive pool
    and the second normalisation, which are identities at 224 x 224."""
    pooled = [F.normalize(F.max_pool2d(t, win, stride).float(), p=2, dim=1) for t, win, stride in zip(taps, il.TAP_WINDOWS, il.TAP_STRIDES)]
    x = torch.cat(pooled, dim=1)
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, il.L3IMAC_DIMS)
    return F.normalize(x, p=2, dim=-1)


fast_stage = il.FastL3iMAC.regions  # four pools + the row normalisation


def timed(fn, taps, reps):
    for _ in range(3):
        fn(taps)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn(taps)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=512)
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--packed-batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check-videos", type=int, default=16)
    ap.add_argument("--stage-reps", type=int, default=50)
    ap.add_argument("--legs", default="fp32-eager,bf16-autocast,FastL3iMAC")
    ap.add_argument("--stage-only", action="store_true", help="skip the end-to-end legs: the region stage alone")
    ap.add_argument("--no-stage", action="store_true", help="skip the region stage's own timing: the end-to-end legs alone")
    args = ap.parse_args()
    assert args.size == 224 or args.no_stage, "the region stage's own timing is written for 224 x 224 (every tap on the final grid)"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no CPU fallback"
    dev = torch.device("cuda", 0)
    model = il.build_l3imac_model(device=dev)
    folded = fold_batchnorm(model).to(memory_format=torch.channels_last)
    fast = il.FastL3iMAC(model).to(dev).eval()
    legs = {
        "fp32-eager": lambda s: run_inference(model, s, dev, 32, None, channels_last=False),
        "bf16-autocast": lambda s: run_inference_packed(folded, s, dev, args.packed_batch, torch.bfloat16, channels_last=True),
        "FastL3iMAC": lambda s: run_inference_packed(fast, s, dev, args.packed_batch, None, channels_last=True),
    }
    names = [n for n in args.legs.split(",") if n]
    src = SyntheticVideos(n_videos=args.videos, frames=(args.frames, args.frames), size=args.size, seed=2)
    warm = SyntheticVideos(n_videos=16, frames=(args.frames, args.frames), size=args.size, seed=3)
    check = SyntheticVideos(n_videos=args.check_videos, frames=(args.frames, args.frames), size=args.size, seed=2)
    rates = {n: [] for n in names}
    if not args.stage_only:
        for n in names:
            for _ in legs[n](warm):
                pass
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for n in names:
                if n == "fp32-eager" and r > 0:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                frames = 0
                for _, d in legs[n](src):
                    frames += d.shape[0]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rates[n].append(frames / dt)
                print(f"round {r} {n:13s}: {frames} frames in {dt:7.2f} s = {frames / dt:9.1f} frames/s", flush=True)
        if "fp32-eager" in names:
            ref = to_flat(legs["fp32-eager"](check))[0]
            for n in names:
                if n != "fp32-eager":
                    cos = F.cosine_similarity(ref, to_flat(legs[n](check))[0], dim=-1)
                    print(f"{n:13s} vs fp32-eager on {check.n_videos} videos (random-init, uncalibrated trunk): min cosine per region "
                          f"{cos.min().item():.6f} mean {cos.mean().item():.6f}")

    if args.no_stage:
        return
    # the region stage alone, on the bf16 NHWC taps of one packed batch
    b =args.packed_batch
    x = preprocess(torch.cat([src.video(i, args.frames, dev) for i in range(-(-b // args.frames))])[:b])
    with torch.no_grad():
        with torch.cuda.device(dev):
            taps = fast.taps(x)
        t_fast = timed(fast_stage, taps, args.stage_reps)
        t_torch = timed(torch_stage, taps, args.stage_reps)
        agree = F.cosine_similarity(fast_stage(taps), torch_stage(taps), dim=-1).min().item()
    nbytes = stage_bytes(b, args.size)
    print(f"region stage, batch {b} at {args.size} x {args.size}: algorithmic bytes {nbytes} ({nbytes / 1e6:.1f} MB)")
    print(f"  kernels (4 x vsc_region_pool_l2_bf16 + vsc_rows_l2norm_f32): {t_fast * 1e6:8.1f} us per batch by device events "
          f"(launch gaps included) = {nbytes / t_fast / 1e12:.2f} TB/s = {100 * nbytes / t_fast / HBM_COPY_RATE:.1f} % of the "
          f"{HBM_COPY_RATE / 1e12:.2f} TB/s copy rate")
    print(f"  torch ops on the same bf16 taps:                               {t_torch * 1e6:8.1f} us per batch   "
          f"(x{t_torch / t_fast:.2f}); min cosine between the two {agree:.7f}")
    if rates.get("FastL3iMAC"):
        per_batch = b / (sum(rates["FastL3iMAC"]) / len(rates["FastL3iMAC"]))
        print(f"  share of FastL3iMAC's forward pass ({per_batch * 1e3:.2f} ms per batch of {b}, end to end): {100 * t_fast / per_batch:.2f} %")


if __name__ == "__main__":
    main()
