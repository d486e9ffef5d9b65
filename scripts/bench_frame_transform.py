#!/usr/bin/env python3
"""Frame transform and packed batches of the inference CLI, timed on the device (profiles/frame_transform.md).

(a) per transform, 128 frames of 360 x 640 and 32 frames of 1080 x 1920, uint8 HWC in HBM -> bf16 NHWC network input:
    the per-batch route of `run_inference` (`device_transform`, then `.to(bfloat16).contiguous(channels_last)` as
    `FastTrunk` does) against `frame_transform.transform_device(out="bf16")`.  Device events around each call, the two
    routes alternating in one process, medians after warm-up; bytes = source read once + output written once; the
    share is that byte rate over the rate of a device-to-device copy measured in the same run.
(b) frames/s of `inference_cli.run_inference` (--batch_size 32) against `inference_cli.run_inference_packed` (128) on
    a synthetic NPY dataset (256 videos x 25 frames of 360 x 640) with a random-init `FastSSCD` behind `CheckedFast`:
    host clock around whole runs (every batch ends in a copy to the host), runs alternating, medians.

    python scripts/bench_frame_transform.py [--rounds 30] [--videos 256] [--runs 3] [--skip_cli]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vsc2022_amd.vsc.baseline import frame_transform as ft  # noqa: E402
from vsc2022_amd.vsc.baseline import inference_cli as cli  # noqa: E402
from vsc2022_amd.vsc.baseline.inference import FastSSCD, build_sscd_model  # noqa: E402


def timed(fn, rounds, warmup=5):
    """Per-call device times in ms of each function in `fn`, the functions alternating inside every round."""
    for _ in range(warmup):
        for f in fn:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fn]
    for _ in range(rounds):
        for i, f in enumerate(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return times


def copy_rate(rounds):
    """Bytes read + written per second of a 1 GiB device-to-device copy."""
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    (t,) = timed([lambda: dst.copy_(src)], rounds)
    return 2.0 * src.numel() / (statistics.median(t) * 1e-3)


def bench_transform(rounds):
    rate = copy_rate(max(5, rounds // 3))
    print(f"device-to-device copy of 1 GiB: {rate / 1e12:.2f} TB/s (read + written)")
    rows = []
    for n, h, w in ((128, 360, 640), (32, 1080, 1920)):
        frames = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda").random_(0, 256)
        for t in cli.InferenceTransforms:
            _, _, _, _, oh, ow = ft.resize_plan(t, h, w)

            def parent():
                return cli.device_transform(frames.permute(0, 3, 1, 2), t).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

            def kernel():
                return ft.transform_device([frames], t, out="bf16")

            # the two routes give the same input up to the parent's documented two 0..255 levels
            step = 1.0 / 255.0 / 0.224
            diff = (parent().float() - kernel().float()).abs().max().item()
            assert diff <= 2.01 * step + 0.02, (t, diff)   # + bf16's rounding of values up to 2.7
            tp, tk = timed([parent, kernel], rounds)
            nbytes = n * h * w * 3 + n * oh * ow * 3 * 2
            mp, mk = statistics.median(tp), statistics.median(tk)
            row = dict(frames=n, source=[h, w], transform=t.name, output=[oh, ow], bytes=nbytes,
                       parent_ms=round(mp, 4), parent_min_ms=round(min(tp), 4), kernel_ms=round(mk, 4), kernel_min_ms=round(min(tk), 4),
                       speedup=round(mp / mk, 2), kernel_GBps=round(nbytes / (mk * 1e-3) / 1e9, 1),
                       share_of_copy_rate=round(nbytes / (mk * 1e-3) / rate, 3))
            rows.append(row)
            print(f"{n:4d} x {h}x{w} {t.name:18s} -> {oh}x{ow}: parent {mp:8.3f} ms  kernel {mk:8.3f} ms  x{mp / mk:6.2f}  "
                  f"{row['kernel_GBps']:8.1f} GB/s = {100 * row['share_of_copy_rate']:.1f} % of the copy rate")
    return dict(copy_rate_TBps=round(rate / 1e12, 3), transform=rows)


def bench_cli(videos, runs):
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        for v in range(videos):
            np.save(os.path.join(d, f"Q{v:06d}.npy"), rng.integers(0, 256, (25, 360, 640, 3), dtype=np.uint8))
        args = cli.build_parser().parse_args(["--accelerator", "cuda", "--fast", "--dataset_path", d, "--video_extensions", "npy",
                                              "--video_reader", "NPY", "--output_file", os.path.join(d, "unused.npz")])
        device = torch.device("cuda", 0)
        transform = cli.InferenceTransforms[args.transforms]

        def dataset():
            return cli.VideoDataset(d, fps=1, extensions=("npy",), video_reader=cli.VideoReaderType.NPY)

        routes = {
            "run_inference --batch_size 32": lambda m: cli.run_inference(dataset(), m, device, transform, 32, False),
            "run_inference_packed 128": lambda m: cli.run_inference_packed(dataset(), m, device, transform, 128, False),
        }

        def model():
            # random-init SSCD, the last BatchNorm scale of every block at 0.25 as the CLI's --fast test sets it: the
            # bf16 network then passes the CheckedFast gate, as a trained checkpoint does
            eager = build_sscd_model(device=device, channels_last=False)
            for blk in eager.trunk:
                blk.bn3.weight.fill_(0.25)
            return cli.CheckedFast(FastSSCD(eager).to(device).eval(), eager, args.fast_min_cosine).eval()

        models = {k: model() for k in routes}
        times = {k: [] for k in routes}
        for r in range(runs + 1):          # the first round warms up (and passes the CheckedFast gate)
            for k, route in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = sum(len(v.feature) for v in route(models[k]))
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert n == videos * 25 and models[k].use_fast
                if r:
                    times[k].append(dt)
        out = {}
        for k, t in times.items():
            out[k] = dict(frames=videos * 25, median_s=round(statistics.median(t), 3), min_s=round(min(t), 3),
                          frames_per_s=round(videos * 25 / statistics.median(t), 1))
            print(f"{k:32s}: {out[k]['frames_per_s']:9.1f} frames/s (median of {runs} runs of {videos * 25} frames, best {min(t):.3f} s)")
        return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rounds", type=int, default=30)
    p.add_argument("--videos", type=int, default=256)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--skip_cli", action="store_true")
    a = p.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the device: there is nothing to time without one"
    res = bench_transform(a.rounds)
    if not a.skip_cli:
        res["cli"] = bench_cli(a.videos, a.runs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
