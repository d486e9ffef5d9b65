#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X matching engine.

metric   : query-videos localized/sec @ 512-d SSCD descriptors (BASELINE.json)
workload : (default, `--scaling strong`) BASELINE.json configs[3] -- the configuration the metric is quoted on: the
           full pipeline incl. score normalisation + TN localisation on 40000 query videos x 25 frames (1M frames,
           split over the N GPUs) against 2M reference frames (40000 videos x 50) and a 2M-row noise set, 512-d fp32,
           L2-normalised, 20% planted copies, 1% static videos.  One step = one query set through the whole hot path
           (vsc/baseline/sscd_baseline.py:185-231): score normalisation of the queries (row L2 + 1-NN against the
           noise index, beta 1.2) -> global-threshold search (K = 1200/video) -> (query, ref) max aggregation ->
           top 25/video candidates -> Temporal-Network localisation (bias 0.5) of the top 5/video pairs.
           `--scaling weak`: BASELINE configs[1]'s shape per GPU (8000 query videos = 200k frames, no score
           normalisation); at N = 1 the default run reports it under "extra".
           All inputs are resident in HBM before the timed region (synthetic, generated on device).
multi-GPU: one process per GPU, queries sharded, references replicated, the two global cuts resolved over RCCL
           (vsc2022_amd/dist.py).  `--gpus N` without a launcher re-executes itself under
           `python -m torch.distributed.run --nproc-per-node N` (127.0.0.1 rendezvous, free port); under
           torchrun it reads RANK / LOCAL_RANK / WORLD_SIZE.  Two scalings:
             --scaling weak   every rank brings its own 8000 query videos (configs[1] shape per GPU);
             --scaling strong (default) BASELINE configs[3] as written: 40000 query videos (1M frames) split N ways,
                              score normalisation against a 2M-row noise set INSIDE the timed step
                              (vsc/baseline/sscd_baseline.py:193-204), 2M reference frames replicated.

Prints ONE JSON line on rank 0: metric, value, unit, higher_is_better, dtype and ms_per_step (milliseconds per timed
step) of the headline.  A plain run does only that: set-up, --warmup steps, --steps timed steps, the line.
`--dump-outputs DIR` then writes what the last timed step returned to its caller (candidate table, localised segments,
final radius) as DIR/<name>.npy, float32 / float64, below 64 MB in all (a fixed, seeded sample of rows beyond that).
`--full` adds "result_digest" (sha256 of that result), "roofline" (the dominant kernel, measured live with HIP events
on the engine's stream during the timed steps), "kernels" (every kernel class of a step: ms, achieved TFLOP/s or GB/s
against its peak), at N > 1 "sharded_search" and a cross-rank check of the candidate tables, and at N=1
"extra" (untimed legs after the headline measurement: BASELINE configs[1]'s shape -- 8000 query videos x 2M reference
frames without score normalisation, a few steps --, its 200k x 2M k-NN as written, query-set upload, score
normalisation of 200k rows, one search on the all-fp32 route) and
"cpu_baseline" (the reference's CPU flow restated on the host BLAS, bounded sample, all host cores).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: dense fp32 matrix rate
FP16_MFMA_PEAK_TFLOPS = 2500.0  # same guide: dense fp16/bf16 matrix rate (sparsity figures excluded)
INT8_MFMA_PEAK_TOPS = 5000.0    # same guide: int8 runs at 2x the bf16 rate (= the dense FP8 figure, ~5 P op/s)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--query-videos", type=int, default=8000, help="query videos per GPU")
    ap.add_argument("--query-frames", type=int, default=25)
    ap.add_argument("--ref-videos", type=int, default=40000)
    ap.add_argument("--ref-frames", type=int, default=50)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--full", action="store_true",
                    help="also report the result digest, per-kernel / roofline figures, the untimed extra legs and the "
                         "CPU baseline (a plain run prints the headline alone)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, < 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the untimed k-NN / score-norm / all-fp32 legs")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="strong",
                    help="weak: --query-videos per GPU (configs[1] shape); strong: --total-query-videos split over the "
                         "GPUs with score normalisation in the timed step (configs[3])")
    ap.add_argument("--total-query-videos", type=int, default=40000, help="--scaling strong: query videos of the whole job")
    ap.add_argument("--noise-rows", type=int, default=0, help="score-normalisation noise rows (default: as many as references)")
    ap.add_argument("--data", default="gaussian",
                    choices=("gaussian", "clusters", "powerlaw", "offset", "temporal", "neardup"),
                    help="distribution class of the synthetic descriptors (vsc2022_amd/synth.py); the headline is gaussian")
    ap.add_argument("--launch-check", action="store_true",
                    help="only launch the ranks, form the process group (gloo, no GPU needed) and report it")
    return ap.parse_args()


def self_launch(args):
    """`bench.py --gpus N` started without a launcher: run N ranks of this script under torch.distributed.run on
    this node (what the reference's inference CLI does with torch.multiprocessing, vsc/baseline/inference.py:107-131)."""
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between processes needs it on this driver
    env["VSC_BENCH_SELF_LAUNCHED"] = "1"
    return subprocess.call(cmd, env=env)


def process_group_check(torch, dist, world, rank, local_rank, dev, share_gpu):
    """Every rank must see `world` ranks of the expected backend, one per device (a mis-launched job would otherwise
    time collectives out minutes later).  Returns what rank 0 reports."""
    assert dist.get_world_size() == world and dist.get_rank() == rank
    on_cpu = share_gpu or dev is None
    seen = torch.zeros(world, dtype=torch.int64, device="cpu" if on_cpu else dev)
    seen[rank] = 1 + local_rank
    dist.all_reduce(seen)
    assert int((seen > 0).sum()) == world, f"rank {rank}: only {int((seen > 0).sum())} of {world} ranks answered"
    if not on_cpu:
        assert dist.get_backend() == "nccl" and len(set(seen.tolist())) == world, \
            f"ranks do not sit on distinct devices of this node: {seen.tolist()}"
    return {"backend": dist.get_backend(), "ranks_answered": int((seen > 0).sum()),
            "devices": [int(v) - 1 for v in seen.tolist()],
            "launcher": "bench.py self-launch" if os.environ.get("VSC_BENCH_SELF_LAUNCHED") == "1" else "external"}


def synth_on_device(torch, dev, seed, n_vid, frames, dim, static_frac=0.01, dist="gaussian", geometry=None,
                    duplicates=False):
    """[n_vid * frames, dim] unit rows in HBM (vsc2022_amd/synth.py:device_rows): a function of the seed and the shape
    alone.  dist: the distribution class (--data); "gaussian" is the generator every earlier round measured."""
    from vsc2022_amd import synth

    return synth.device_rows(torch, dev, seed, n_vid, frames, dim, static_frac, dist, geometry, duplicates)


def plant_copies(torch, dev, seed, q, n_qvid, qf, r, n_rvid, rf, frac=0.2, noise=0.05):
    """For `frac` of the query videos overwrite a run of frames with a noised reference segment."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    n_planted = int(round(frac * n_qvid))
    qv = torch.randperm(n_qvid, generator=g)[:n_planted]
    rv = torch.randint(0, n_rvid, (n_planted,), generator=g)
    length = torch.randint(8, min(qf, rf, 25) + 1, (n_planted,), generator=g)
    q0 = (torch.rand(n_planted, generator=g) * (qf - length + 1).float()).long()
    r0 = (torch.rand(n_planted, generator=g) * (rf - length + 1).float()).long()
    gd = torch.Generator(device=dev)
    gd.manual_seed(seed + 1)
    gt = []
    for k in range(n_planted):
        L = int(length[k])
        qs = int(qv[k]) * qf + int(q0[k])
        rs = int(rv[k]) * rf + int(r0[k])
        seg = r[rs : rs + L] + noise * torch.randn((L, q.shape[1]), generator=gd, device=dev)
        q[qs : qs + L] = seg / seg.norm(dim=1, keepdim=True)
        gt.append((int(qv[k]), int(rv[k])))
    return gt


def result_digest(torch, matcher, res):
    """What the job computed, as hashes that do not depend on the number of ranks: sha256 over the schedule's final
    radius, the candidate table (query video, reference video, score bits -- vsc/baseline/sscd_baseline.py:98-115) and
    the gathered table of localised segments (candidate, box, MaxSim bits -- :139-152), in the single-process order.
    `--gpus 1` and `--gpus N` runs of the same command line must print the same `result_digest`."""
    import hashlib

    boxes = matcher.gather_boxes(res)
    parts = {
        "radius": np.array([res.radius], dtype=np.float32).tobytes(),
        "candidates": b"".join(t.contiguous().cpu().numpy().tobytes() for t in
                               (res.cand_q.to(torch.int32), res.cand_r.to(torch.int32),
                                res.cand_score.contiguous().view(torch.int32))),
        "boxes": boxes.contiguous().cpu().numpy().tobytes(),
    }
    whole = hashlib.sha256()
    out = {}
    for k, v in parts.items():
        whole.update(v)
        out[k] = hashlib.sha256(v).hexdigest()[:16]
    return {"result_digest": whole.hexdigest()[:32], "parts": out, "n_boxes": int(boxes.shape[0]),
            "tie_on_cut": bool(res.tie_on_cut), "ties_dropped": bool(res.ties_dropped)}


DUMP_BYTES = 60_000_000  # --dump-outputs: payload bound, so that the files stay below 64 MB with their headers


def output_arrays(torch, matcher, res):
    """What a caller of the timed path receives from its last step, as float64 (integers, exact below 2**53) and float32
    (scores) arrays: the candidate table (query video, reference video, score), the localised segments (index into the
    candidate table, q_lo, r_lo, q_hi, r_hi, MaxSim - bias) in the single-process order, and the final radius.  The
    segment table is gathered over the ranks (a collective at N > 1: every rank calls this)."""
    boxes = matcher.gather_boxes(res)
    return {
        "radius": np.array([res.radius], dtype=np.float32),
        "cand_query": res.cand_q.cpu().numpy().astype(np.float64),
        "cand_ref": res.cand_r.cpu().numpy().astype(np.float64),
        "cand_score": res.cand_score.cpu().numpy().astype(np.float32),
        "box_cand": boxes[:, 0].cpu().numpy().astype(np.float64),
        "box_coords": boxes[:, 1:5].cpu().numpy().astype(np.float64),
        "box_score": boxes[:, 5].to(torch.int32).cpu().numpy().view(np.float32),
    }


def dump_outputs(path, arrays):
    """DIR/<name>.npy for every array.  Above DUMP_BYTES in all, every array keeps the same share of its rows, a fixed
    seeded sample (arrays of one length keep the same rows, so the tables stay aligned)."""
    os.makedirs(path, exist_ok=True)
    frac = min(1.0, DUMP_BYTES / max(1, sum(a.nbytes for a in arrays.values())))
    for name, a in arrays.items():
        if frac < 1.0 and a.shape[0] > 1:
            keep = np.random.default_rng(0).choice(a.shape[0], max(1, int(a.shape[0] * frac)), replace=False)
            a = a[np.sort(keep)]
        np.save(os.path.join(path, f"{name}.npy"), np.ascontiguousarray(a))


def host_cores() -> int:
    """The host cores this process may really use -- the affinity mask cut by the cgroup CPU quota (a pod on a 256-core
    host sees every core in its mask; a thread team that size on a 16-core quota spends its time being throttled):
    ONE figure for every CPU leg."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                quota = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                period = int(f.read())
            if quota > 0 and period > 0:
                n = min(n, max(1, quota // period))
        except (OSError, ValueError):
            pass
    return max(1, n)


def cpu_baseline(args, strong):
    """The reference's CPU path restated on the host BLAS, whole flow, bounded sample, all host cores:

      score normalisation   row L2 + 1-NN against the noise rows as blocked sgemm + row max (what FAISS's CPU flat
                            index does for `index.search(x, 1)`, vsc/baseline/score_normalization.py:93-99)
      search                faiss.contrib.exhaustive_search.range_search_max_results over the doubling batches
                            (vsc/index.py:147-154): blocked sgemm + strict threshold, (K+1)-th best re-thresholds,
                            stable sort, cut at K
      candidates            per-pair max in first-appearance order, vectorised (vsc/candidates.py:24-40)
      localisation          per pair sims = a @ b.T + bias, Temporal Network from the C oracle, pairs spread over a
                            thread pool (the reference: a 16-process pool, vsc/baseline/sscd_baseline.py:118-135)

    Scores come out of the BLAS's summation order, so this leg checks nothing; it says what the host cores deliver on
    this flow.  A few hundred query videos against 1/10 of the reference and noise rows; per-query cost is linear in
    those rows, the rate is scaled by that 1/10.  (The fma-chain port that the parity tests use is timed separately:
    `cpu_baseline_exact_port`.)"""
    from concurrent.futures import ThreadPoolExecutor

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as orc

    orc.build()
    cores = host_cores()
    try:
        from threadpoolctl import threadpool_limits

        limiter = threadpool_limits(limits=cores)
    except Exception:
        limiter = None
    orc.set_num_threads(cores)
    rng = np.random.default_rng(args.seed)
    dim, qf, rf = args.dim, args.query_frames, args.ref_frames
    n_rv = max(1, args.ref_videos // 10)
    n_noise = max(1, (args.noise_rows or args.ref_videos * args.ref_frames) // 10)
    nr = n_rv * rf
    def unit(n):
        x = rng.standard_normal((n, dim)).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    # ~15-20 s whatever the host: the sample is sized from the sgemm rate these cores deliver (a 0.2 s probe); thresholds,
    # selection and sorting take the flow to ~3x its pure sgemm time
    probe_a, probe_b = unit(1024), unit(8192)
    (probe_a @ probe_b.T).sum()
    t_probe = time.perf_counter()
    (probe_a @ probe_b.T).sum()
    rate = 2.0 * 1024 * 8192 * dim / max(time.perf_counter() - t_probe, 1e-6)
    per_video = 2.0 * qf * (nr + (n_noise if strong else 0)) * dim
    n_qv = int(min(8192, max(64, 9.0 * rate / per_video)))

    q, r = unit(n_qv * qf), unit(nr)
    for v in range(0, n_qv, 5):  # planted copies
        rv = int(rng.integers(0, n_rv))
        q[v * qf : v * qf + 12] = r[rv * rf + 3 : rv * rf + 15]
    row2q = np.repeat(np.arange(n_qv, dtype=np.int64), qf)
    row2r = np.repeat(np.arange(n_rv, dtype=np.int64), rf)
    bias = 0.0
    if strong:
        # the reference side of the score normalisation is resident state (as on the GPU); the query side is timed
        noise = unit(n_noise)
        keep = np.delete(np.arange(dim), int(np.argmin(noise.var(axis=0))))
        noise_n = noise[:, keep] / np.linalg.norm(noise[:, keep], axis=1, keepdims=True)
        rk = r[:, keep] / np.linalg.norm(r[:, keep], axis=1, keepdims=True)
        r = np.ascontiguousarray(np.concatenate([rk, np.ones((nr, 1), np.float32)], axis=1))
        bias = 0.5
    K = 1200 * n_qv
    BLOCK = 2048  # query rows per sgemm (FAISS blocks its flat search the same way)
    stage = {}
    t0 = time.perf_counter()
    if strong:
        qn = q[:, keep] / np.linalg.norm(q[:, keep], axis=1, keepdims=True)
        best = np.empty(len(qn), dtype=np.float32)
        for a in range(0, len(qn), BLOCK):
            best[a : a + BLOCK] = (qn[a : a + BLOCK] @ noise_n.T).max(axis=1)
        q = np.ascontiguousarray(np.concatenate([qn, (-1.2 * best).reshape(-1, 1)], axis=1))
    stage["score_norm_s"] = time.perf_counter() - t0
    # ---- range_search_max_results over exponential_query_iterator
    t1 = time.perf_counter()
    radius, kept, total, bs, i0, nq = np.float32(-1e10), [], 0, 32, 0, len(q)
    while i0 < nq:
        i1 = min(nq, i0 + bs)
        for a in range(i0, i1, BLOCK):
            b = min(i1, a + BLOCK)
            S = q[a:b] @ r.T
            ii, jj = np.nonzero(S > radius)
            kept.append((ii + a, jj, S[ii, jj]))
            total += len(ii)
        if total > 2 * K:
            alls = np.concatenate([k[2] for k in kept])
            radius = np.partition(alls, len(alls) - K - 1)[len(alls) - K - 1]
            kept = [(ki[ks > radius], kj[ks > radius], ks[ks > radius]) for ki, kj, ks in kept]
            total = sum(len(k[2]) for k in kept)
        if bs < 20000:
            bs *= 2
        i0 = i1
    hi = np.concatenate([k[0] for k in kept])
    hj = np.concatenate([k[1] for k in kept])
    hs = np.concatenate([k[2] for k in kept])
    order = np.argsort(-hs, kind="stable")[:K]
    hi, hj, hs = hi[order], hj[order], hs[order]
    stage["search_s"] = time.perf_counter() - t1
    # ---- per-pair max, first-appearance order; best 25 / 5 per query video
    t2 = time.perf_counter()
    key = row2q[hi] * n_rv + row2r[hj]
    _, first = np.unique(key, return_index=True)
    first.sort()
    pq, pr = row2q[hi[first]], row2r[hj[first]]
    n_loc = min(len(first), 5 * n_qv)
    stage["pair_max_s"] = time.perf_counter() - t2
    # ---- Temporal Network on the best pairs
    t3 = time.perf_counter()

    def localise(span):
        n = 0
        for k in range(*span):
            a = q[pq[k] * qf : (pq[k] + 1) * qf]
            b = r[pr[k] * rf : (pr[k] + 1) * rf]
            n += len(orc.tn((a @ b.T + np.float32(bias)).astype(np.float32), tn_max_step=5, min_length=4))
        return n

    step = max(1, n_loc // (4 * cores) + 1)
    with ThreadPoolExecutor(max_workers=cores) as pool:
        n_boxes = sum(pool.map(localise, [(a, min(n_loc, a + step)) for a in range(0, n_loc, step)]))
    stage["tn_s"] = time.perf_counter() - t3
    dt = time.perf_counter() - t0
    if limiter is not None:
        limiter.restore_original_limits()
    scale = nr / float(args.ref_videos * args.ref_frames)
    flops = 2.0 * len(q) * (nr + (n_noise if strong else 0)) * dim
    return {
        "value": (n_qv / dt) * scale,
        "unit": "query-videos/s",
        "cores": cores,
        "kind": "port",
        "restatement": "BLAS: blocked sgemm + strict threshold / row max (FAISS's CPU flat index), numpy pair-max, C-oracle "
                       "Temporal Network on a thread pool -- the whole " + ("configs[3]" if strong else "configs[1]") + " flow",
        "sgemm_tflops": flops / max(stage["score_norm_s"] + stage["search_s"], 1e-9) / 1e12,
        "stage_seconds": {k: round(v, 3) for k, v in stage.items()},
        "sample": f"{n_qv} query videos x {qf} frames vs {nr} ref frames"
                  + (f" + score normalisation against {n_noise} noise rows" if strong else "")
                  + f" ({dim}-d): {len(hs)} hits, {len(first)} pairs, {n_loc} localised, {n_boxes} segments in {dt:.2f} s on "
                    f"{cores} cores; rate scaled by {scale:.3f} (per-query cost is linear in ref / noise rows)",
    }


def cpu_baseline_exact_port(args, strong):
    """The C oracle (oracle/libvscoracle.so: OpenMP, AVX2 fma chains) on the host cores over a bounded sample of
    the same workload: a few dozen query videos against 1/10 of the references (and, for configs[3], 1/10 of the
    noise rows for the score normalisation of the sample).  Per-query cost is linear in the number of reference /
    noise rows, so the rate is scaled by that 1/10."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as orc

    orc.build()
    orc.set_num_threads(host_cores())  # the same cores as `cpu_baseline`
    rng = np.random.default_rng(args.seed)
    # ~10-15 s of CPU work whatever the core count (0.2 s per query video per core at this size)
    n_qv, qf = max(48, min(256, 4 * orc.num_threads())), args.query_frames
    n_rv, rf = max(1, args.ref_videos // 10), args.ref_frames
    n_noise = max(1, (args.noise_rows or args.ref_videos * args.ref_frames) // 10)
    dim = args.dim

    def unit(n):
        x = rng.standard_normal((n, dim)).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    q, r = unit(n_qv * qf), unit(n_rv * rf)
    for v in range(0, n_qv, 5):  # planted copies
        rv = int(rng.integers(0, n_rv))
        q[v * qf : v * qf + 12] = r[rv * rf + 3 : rv * rf + 15]
    row2q = np.repeat(np.arange(n_qv, dtype=np.int32), qf)
    row2r = np.repeat(np.arange(n_rv, dtype=np.int32), rf)
    threads = orc.num_threads()
    bias = 0.0
    if strong:
        # the reference side of the score normalisation is resident state (as on the GPU); the query side is timed
        noise = unit(n_noise)
        keep = np.delete(np.arange(dim), int(np.argmin(noise.var(axis=0))))
        noise_n = orc.row_normalize(noise[:, keep])
        r = np.concatenate([orc.row_normalize(r[:, keep]), np.ones((len(r), 1), np.float32)], axis=1)
        bias = 0.5
    t0 = time.perf_counter()
    if strong:
        # vsc/baseline/score_normalization.py:31-105 on the sample: drop the weakest dim, row L2, -beta * 1-NN vs noise
        qn = orc.row_normalize(q[:, keep])
        best, _ = orc.knn(qn, noise_n, 1)
        q = np.concatenate([qn, -1.2 * np.asarray(best, dtype=np.float32).reshape(-1, 1)], axis=1)
    hi, hj, hs = orc.global_threshold_search(q, r, 1200 * n_qv)
    pq, pr, ps, _ = orc.pair_max(hi, hj, hs, row2q, row2r)
    n_loc = min(len(ps), 5 * n_qv)
    n_boxes = 0
    for k in range(n_loc):
        a = q[pq[k] * qf : (pq[k] + 1) * qf]
        b = r[pr[k] * rf : (pr[k] + 1) * rf]
        n_boxes += len(orc.tn(orc.pair_sims(a, b, bias), tn_max_step=5, min_length=4))
    dt = time.perf_counter() - t0
    scale = (n_rv * rf) / float(args.ref_videos * args.ref_frames)
    return {
        "value": (n_qv / dt) * scale,
        "unit": "query-videos/s",
        "cores": threads,
        "kind": "port",
        "sample": f"{n_qv} query videos x {qf} frames vs {n_rv * rf} ref frames"
                  + (f" + score normalisation against {n_noise} noise rows" if strong else "")
                  + f" ({dim}-d) in {dt:.2f} s on {threads} threads; rate scaled by {scale:.3f} (per-query cost is "
                    "linear in ref / noise rows)",
    }


HBM_PEAK_GBS = 8000.0  # same guide: HBM3E peak (6.3 TB/s is what a copy kernel achieves)


def _aux(cls):
    """(ms, calls, bytes) of the process-wide accounting: 0 = pair-max, 1 = Temporal Network."""
    import ctypes

    from vsc2022_amd import _lib

    ms, n, by = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0)
    _lib.check(_lib.lib().vsc_aux_profile_read(cls, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(by), 1))
    return ms.value, n.value, by.value


def _rate(work, ms, scale):
    return (work / scale) / (ms / 1e3) if ms > 0 else 0.0


def extra_legs(args, torch, dev, matcher, queries, n_qv, qf, n_rv, rf, dim):
    """Untimed legs of the single-GPU run (after the headline measurement, bounded to a few seconds each): every
    figure DESIGN.md quotes comes from here or from a tracked profile."""
    import time as _t

    from vsc2022_amd import _lib
    from vsc2022_amd.engine import DeviceScoreNormalizer
    from vsc2022_amd.vsc.index import FlatIndex

    out = {}
    nq, nr = n_qv * qf, n_rv * rf
    idx = matcher.index
    # ---- BASELINE configs[1] as written: brute-force cosine k-NN 200k x 2M (index.search, results to the host)
    knn = {}
    for k in (20, 1):
        idx.search(queries, k)  # warm-up at full size (work buffers are allocated on first use)
        idx.profile_read(reset=True)
        torch.cuda.synchronize()
        t0 = _t.perf_counter()
        D, I = idx.search(queries, k)
        dt = _t.perf_counter() - t0
        p = idx.profile_read(reset=True)
        knn[f"k{k}"] = {
            "ms": 1e3 * dt, "query_rows_per_s": nq / dt, "algorithmic_tflops": 2.0 * nq * nr * dim / dt / 1e12,
            "kernel_ms": {"exact_fp32_subset_pass": p["sim_ms"], "int8_prefilter": p["i8_ms"], "int8_preamble": p.get("i8_prep_ms", 0.0),
                          "fp16_prefilter": p["f16_ms"],
                          "exact_rescore": p["rescore_ms"]},
            "prefilter_tops": _rate(p["f16_flops"] + p["i8_flops"], p["f16_ms"] + p["i8_ms"], 1e12),
            "candidates": p["candidates"],
        }
        del D, I
    out["knn_200k_x_2M"] = knn
    # ---- per query set: upload + packing of a fresh query batch (outside the headline's timed region)
    q_off = np.arange(n_qv + 1, dtype=np.int64) * qf
    matcher.set_queries(queries, q_off)
    torch.cuda.synchronize()
    t0 = _t.perf_counter()
    matcher.set_queries(queries, q_off)
    torch.cuda.synchronize()
    out["set_queries_ms"] = 1e3 * (_t.perf_counter() - t0)
    # ---- score normalisation of this query set against a 2M-row noise set (config 4's extra stage)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed + 77)
    noise = torch.randn((nr, dim), generator=g, device=dev, dtype=torch.float32)
    noise /= noise.norm(dim=1, keepdim=True)
    norm = DeviceScoreNormalizer(noise, beta=1.2)
    del noise
    norm.queries(queries[:4096])
    torch.cuda.synchronize()
    t0 = _t.perf_counter()
    qn = norm.queries(queries)
    torch.cuda.synchronize()
    out["score_normalize_queries_ms"] = 1e3 * (_t.perf_counter() - t0)
    out["score_normalize_note"] = (f"{nq} query rows: drop the low-variance dim, row-L2, 1-NN against {nr} noise rows "
                                   "(pre-filtered exact k-NN), beta 1.2; noise index resident")
    del qn, norm
    torch.cuda.empty_cache()
    # ---- the all-fp32 route (option "prefilter" = 0): one search of the same shape on the exact fp32 MFMA kernel alone
    exact = FlatIndex(dim, _lib.METRIC_INNER_PRODUCT, dev.index, options={"prefilter": 0})
    exact.add(matcher.ref_feats)
    exact.profile(True)
    exact.profile_read(reset=True)
    torch.cuda.synchronize()
    t0 = _t.perf_counter()
    hits = exact.global_topk(queries, 1200 * n_qv, device_out=True)
    torch.cuda.synchronize()
    dt = _t.perf_counter() - t0
    p = exact.profile_read(reset=True)
    ach = _rate(p["sim_flops"], p["sim_ms"], 1e12)
    # ... and an exhaustive parity check while both results are in HBM: the default route (fp16 / int8 pre-filters +
    # exact stage) must return the same (row, ref, score bits) list, all K entries of it, and the same radius
    di, dj, ds, drad = matcher.search(1200 * n_qv)
    out["fullsize_routes_identical"] = bool(
        drad == hits[3] and ds.numel() == hits[2].numel() and torch.equal(di, hits[0]) and torch.equal(dj, hits[1])
        and torch.equal(ds.view(torch.int32), hits[2].view(torch.int32)))
    out["fullsize_routes_note"] = (f"default route vs VSC_PREFILTER=0 on the whole {nq} x {nr} score matrix, K = {1200 * n_qv}: "
                                   "every hit's row, reference and fp32 score bits + the final radius compared")
    del di, dj, ds
    out["roofline_fp32_route"] = {
        "kernel": "sim_thresh_kernel (fp32 MFMA 32x32x2 similarity + fused threshold compaction), VSC_PREFILTER=0",
        "bound": "mfma", "achieved": ach, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
        "frac": ach / FP32_MFMA_PEAK_TFLOPS, "launches": p["sim_launches"], "kernel_ms": p["sim_ms"],
        "search_ms": 1e3 * dt, "hits": int(hits[2].numel()),
    }
    del exact, hits
    torch.cuda.empty_cache()
    return out


def config2_shape_leg(args, torch, dev, dim):
    """BASELINE configs[1]'s shape on this one GPU, untimed extra leg of the default run: 8000 query videos x 25
    frames (200k rows) against the 2M reference frames, no score normalisation -- the hot path of one query set
    (search K = 9.6M -> 200k candidates -> 40k pairs localised), a few steps; then the legs of `extra_legs` on the
    same matcher (the 200k x 2M k-NN as written, query upload, score normalisation of 200k rows, all-fp32 route)."""
    import time as _t

    from vsc2022_amd.engine import DeviceMatcher

    n_qv, qf, n_rv, rf = args.query_videos, args.query_frames, args.ref_videos, args.ref_frames
    refs = synth_on_device(torch, dev, args.seed, n_rv, rf, dim)
    queries = synth_on_device(torch, dev, args.seed + 1000, n_qv, qf, dim)
    plant_copies(torch, dev, args.seed + 2000, queries, n_qv, qf, refs, n_rv, rf)
    m = DeviceMatcher(refs, np.arange(n_rv + 1, dtype=np.int64) * rf, dev.index)
    del refs
    m.set_queries(queries, np.arange(n_qv + 1, dtype=np.int64) * qf)
    m.match()
    m.index.profile(True)
    m.index.profile_read(reset=True)
    _aux(0), _aux(1)
    steps = 3
    torch.cuda.synchronize()
    t0 = _t.perf_counter()
    for _ in range(steps):
        res = m.match()
    torch.cuda.synchronize()
    dt = (_t.perf_counter() - t0) / steps
    p = m.index.profile_read(reset=True)
    tn_ms = _aux(1)[0] / steps
    out = {
        "workload": f"BASELINE configs[1] shape: {n_qv} query videos ({n_qv * qf} frames) vs {n_rv * rf} reference frames, "
                    f"{dim}-d, no score normalisation, {steps} steps",
        "ms_per_step": 1e3 * dt, "query_videos_per_s": n_qv / dt, "hits": res.n_hits, "candidates": res.n_candidates,
        "pairs_localized": res.n_localized, "matches": res.n_matches,
        "kernel_ms_per_step": {"int8_prefilter": p["i8_ms"] / steps, "fp16_prefilter": p["f16_ms"] / steps,
                               "exact_fp32": p["sim_ms"] / steps, "exact_rescore": p["rescore_ms"] / steps,
                               "select": p["select_ms"] / steps, "final_sort": p["sort_ms"] / steps, "tn": tn_ms},
        "int8_prefilter_tops": _rate(p["i8_flops"], p["i8_ms"], 1e12),
    }
    out.update(extra_legs(args, torch, dev, m, queries, n_qv, qf, n_rv, rf, dim))
    ms_fresh = out["ms_per_step"] + out["set_queries_ms"]
    out["value_with_fresh_query_set"] = n_qv / (ms_fresh / 1e3)
    out["value_with_score_norm"] = n_qv / ((ms_fresh + out["score_normalize_queries_ms"]) / 1e3)
    del m, queries
    torch.cuda.empty_cache()
    return out


def distribution_leg(args, torch, dev, dim, dist, score_norm=False, exhaustive=True, steps=2, geo_kw=None):
    """BASELINE configs[1]'s shape (8000 query videos x 25 frames vs 2 M reference frames) on descriptors of another
    distribution class (vsc2022_amd/synth.py): what the pre-filters' bounds, the density rules and
    the 1-NN ranges -- all tuned on isotropic rows -- do on clustered / anisotropic / shifted data.  Reports ms per
    step, candidates handed to the exact stage per emitted hit, launches and ms per route, int8 -> fp16 fall-backs, and
    (exhaustive) whether the default route returns the all-fp32 route's K hits bit for bit."""
    import time as _t

    from vsc2022_amd import _lib, synth
    from vsc2022_amd.engine import DeviceMatcher, DeviceScoreNormalizer
    from vsc2022_amd.vsc.index import FlatIndex

    n_qv, qf, n_rv, rf = args.query_videos, args.query_frames, args.ref_videos, args.ref_frames
    geo = None if dist == "gaussian" else synth.Geometry(dist, dim, args.seed, **(geo_kw or {}))
    refs = synth_on_device(torch, dev, args.seed, n_rv, rf, dim, dist=dist, geometry=geo, duplicates=True)
    queries = synth_on_device(torch, dev, args.seed + 1000, n_qv, qf, dim, dist=dist, geometry=geo)
    gt = plant_copies(torch, dev, args.seed + 2000, queries, n_qv, qf, refs, n_rv, rf)
    out = {"data": dist, "score_normalised": bool(score_norm)}
    if geo_kw:
        out["geometry"] = dict(geo_kw)
    bias = 0.0
    if score_norm:
        noise = synth_on_device(torch, dev, args.seed + 77, n_rv * rf, 1, dim, static_frac=0.0, dist=dist, geometry=geo)
        norm = DeviceScoreNormalizer(noise, beta=1.2)
        del noise
        norm.noise_index.profile(True)
        norm.queries(queries[:4096])
        norm.noise_index.profile_read(reset=True)
        torch.cuda.synchronize()
        t0 = _t.perf_counter()
        queries_n = norm.queries(queries)
        torch.cuda.synchronize()
        out["score_normalize_queries_ms"] = 1e3 * (_t.perf_counter() - t0)
        np_ = norm.noise_index.profile_read(reset=True)
        out["score_normalize_candidates_per_row"] = np_["candidates"] / float(n_qv * qf)
        out["score_normalize_i8_fallbacks"] = int(norm.noise_index.get_option("i8_fallbacks"))
        refs, queries, bias = norm.refs(refs), queries_n, 0.5
        del norm
        torch.cuda.empty_cache()
    m = DeviceMatcher(refs, np.arange(n_rv + 1, dtype=np.int64) * rf, dev.index)
    m.set_queries(queries, np.arange(n_qv + 1, dtype=np.int64) * qf)
    res = m.match(bias=bias)
    m.index.profile(True)
    m.index.profile_read(reset=True)
    _aux(0), _aux(1)
    torch.cuda.synchronize()
    t0 = _t.perf_counter()
    for _ in range(steps):
        res = m.match(bias=bias)
    torch.cuda.synchronize()
    dt = (_t.perf_counter() - t0) / steps
    p = m.index.profile_read(reset=True)
    K = 1200 * n_qv
    planted = set(gt)
    cq, cr = res.cand_q.cpu().numpy(), res.cand_r.cpu().numpy()
    nbox = res.nbox.cpu().numpy()
    loc = set(zip(cq[: res.n_localized][nbox > 0].tolist(), cr[: res.n_localized][nbox > 0].tolist()))
    out.update({
        "ms_per_step": 1e3 * dt, "query_videos_per_s": n_qv / dt, "hits": res.n_hits, "matches": res.n_matches,
        "radius": res.radius, "candidates_per_hit": p["candidates"] / float(max(res.n_hits, 1)),
        "planted_in_candidates": len(planted & set(zip(cq.tolist(), cr.tolist()))) / float(max(len(planted), 1)),
        "planted_localised": len(planted & loc) / float(max(len(planted), 1)),
        "launches_per_step": {"int8": p["i8_launches"] / steps, "fp16": p["f16_launches"] / steps, "exact_fp32": p["sim_launches"] / steps},
        "kernel_ms_per_step": {"int8_prefilter": p["i8_ms"] / steps, "int8_preamble": p.get("i8_prep_ms", 0.0) / steps,
                               "fp16_prefilter": p["f16_ms"] / steps, "exact_fp32": p["sim_ms"] / steps,
                               "exact_rescore": p["rescore_ms"] / steps, "select": p["select_ms"] / steps,
                               "final_sort": p["sort_ms"] / steps, "tn": _aux(1)[0] / steps},
        "int8_prefilter_tops": _rate(p["i8_flops"], p["i8_ms"], 1e12),
        "i8_fallbacks": int(m.index.get_option("i8_fallbacks")),
        "i8_enabled": int(m.index.get_option("i8")),
        # (is the int8 reference image centred on the rows' mean, and the share of the rows' energy that mean carries)
        "i8_center_on": int(m.index.get_option("i8_center_on")), "i8_center_share": m.index.get_option("i8_center_share"),
    })
    if exhaustive:
        exact = FlatIndex(int(refs.shape[1]), _lib.METRIC_INNER_PRODUCT, dev.index, options={"prefilter": 0})
        exact.add(m.ref_feats)
        torch.cuda.synchronize()
        t0 = _t.perf_counter()
        ei, ej, es, erad = exact.global_topk(m.q_feats, K, device_out=True)
        torch.cuda.synchronize()
        out["all_fp32_search_ms"] = 1e3 * (_t.perf_counter() - t0)
        di, dj, ds, drad = m.search(K)
        out["routes_identical"] = bool(drad == erad and ds.numel() == es.numel() and torch.equal(di, ei) and torch.equal(dj, ej)
                                       and torch.equal(ds.view(torch.int32), es.view(torch.int32)))
        del exact, ei, ej, es
    del m, refs, queries
    torch.cuda.empty_cache()
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.launch_check:
        # the launch + rendezvous path alone (tests/test_dist_gloo.py runs it on CPU): no GPU is touched
        pg = {"backend": None, "ranks_answered": 1, "devices": [0], "launcher": "none"}
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo", rank=rank, world_size=world)
            pg = process_group_check(torch, dist, world, rank, local_rank, None, True)
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": world, "gpus_requested": args.gpus, "process_group": pg}),
                  flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (gfx950) GPU: the engine has no CPU fallback")
    # VSC_BENCH_SHARE_GPU=1: debugging aid for a 1-GPU box -- all ranks use cuda:0 and the collectives
    # go over gloo (RCCL cannot place two ranks on one device).  The driver never sets it.
    share_gpu = os.environ.get("VSC_BENCH_SHARE_GPU") == "1"
    if share_gpu:
        local_rank = 0
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    pg = {"backend": None, "ranks_answered": 1, "devices": [local_rank], "launcher": "none"}
    # under a launcher (torch.distributed.run sets WORLD_SIZE) the process group is formed even for ONE rank: the
    # collectives of the timed region and of the final check then run over RCCL exactly as they do for N > 1
    use_dist = world > 1 or "WORLD_SIZE" in os.environ
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        pg = process_group_check(torch, dist, world, rank, local_rank, dev, share_gpu)

    from vsc2022_amd import _lib
    from vsc2022_amd import dist as vdist
    from vsc2022_amd.engine import DeviceMatcher, DeviceScoreNormalizer

    strong = args.scaling == "strong"
    qf, n_rv, rf, dim = args.query_frames, args.ref_videos, args.ref_frames, args.dim
    if strong:
        n_qv_total = args.total_query_videos
        lo, hi = vdist.shard_ranges(n_qv_total, world)[rank]
        n_qv, qv_base = hi - lo, lo
    else:
        n_qv, qv_base = args.query_videos, rank * args.query_videos
        n_qv_total = n_qv * world
    # The WHOLE job's inputs are a function of the seed alone: every rank generates the global query set and keeps its
    # slice, so `--gpus 1` and `--gpus N` see the same data and `result_digest` below can be compared across world sizes
    # ("1-GPU vs 2/4/8-GPU outputs identical")
    from vsc2022_amd import synth

    geo = None if args.data == "gaussian" else synth.Geometry(args.data, dim, args.seed)
    refs = synth_on_device(torch, dev, args.seed, n_rv, rf, dim, dist=args.data, geometry=geo, duplicates=True)
    queries_all = synth_on_device(torch, dev, args.seed + 1000, n_qv_total, qf, dim, dist=args.data, geometry=geo)
    plant_copies(torch, dev, args.seed + 2000, queries_all, n_qv_total, qf, refs, n_rv, rf)
    queries = queries_all[qv_base * qf : (qv_base + n_qv) * qf].clone()
    del queries_all
    r_off = np.arange(n_rv + 1, dtype=np.int64) * rf
    q_off = np.arange(n_qv + 1, dtype=np.int64) * qf
    norm = None
    if strong:
        # configs[3]: both sides score-normalised against the noise set (resident state, like the reference index);
        # the QUERY side of it belongs to every query set and is timed
        noise = synth_on_device(torch, dev, args.seed + 77, args.noise_rows or n_rv * rf, 1, dim, static_frac=0.0,
                                dist=args.data, geometry=geo)
        norm = DeviceScoreNormalizer(noise, beta=1.2)
        del noise
        matcher = DeviceMatcher(norm.refs(refs), r_off, local_rank)
        matcher.set_queries(norm.queries(queries), q_off)
    else:
        matcher = DeviceMatcher(refs, r_off, local_rank)
        matcher.set_queries(queries, q_off)
    del refs
    kw = {}
    if world > 1:
        kw = dict(n_qvid_global=n_qv_total, qvid_base=qv_base, row_base=qv_base * qf)
    if strong:
        kw["bias"] = 0.5

    def step():
        if strong:
            matcher.set_queries(norm.queries(queries), q_off)
        return matcher.match(**kw)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        res = step()
    if args.full:
        # per-kernel accounting (HIP events on the engine's stream) over the timed steps: --full only
        matcher.index.profile(True)
        matcher.index.profile_read(reset=True)
        if norm is not None:
            norm.noise_index.profile(True)
            norm.noise_index.profile_read(reset=True)
        _lib.check(_lib.lib().vsc_aux_profile(1))
        _aux(0), _aux(1)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    barrier()
    dt = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if share_gpu else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs:
        arrays = output_arrays(torch, matcher, res)   # (collective at N > 1: every rank takes part)
        if rank == 0:
            dump_outputs(args.dump_outputs, arrays)
        del arrays
    if args.full:
        prof = matcher.index.profile_read(reset=True)
        nprof = norm.noise_index.profile_read(reset=True) if norm is not None else None
        pm_ms, pm_calls, pm_bytes = _aux(0)
        tn_ms, tn_calls, tn_bytes = _aux(1)
        digest = result_digest(torch, matcher, res)   # (collective at N > 1: every rank takes part, all hold the same tables)
        # the sharded search's phases of the LAST step, max over ranks (dist.PhaseTimer: recorded without synchronising)
        shard_phases = None
        if world > 1 and getattr(matcher, "last_shard_stats", None):
            shard_phases = vdist.reduce_phase_report(matcher.last_shard_stats.get("phases", {}), dev)
    if use_dist and args.full:
        # every rank must hold the same global candidate table (the sharded merge is deterministic)
        h = torch.stack([res.cand_q.to(torch.int64).sum(), res.cand_r.to(torch.int64).sum(),
                         res.cand_score.contiguous().view(torch.int32).to(torch.int64).sum()])
        hs = [torch.zeros_like(h) for _ in range(world)] if not share_gpu else None
        if share_gpu:
            hc = h.cpu()
            hs = [torch.zeros_like(hc) for _ in range(world)]
            dist.all_gather(hs, hc)
        else:
            dist.all_gather(hs, h)
        assert all(torch.equal(x, hs[0]) for x in hs), "candidate tables differ between ranks"
    if rank == 0:
        total_videos = n_qv_total * args.steps
        if strong:
            workload = (f"BASELINE configs[3]: full pipeline incl. score normalisation + TN localisation, {n_qv_total} query "
                        f"videos split over {world} GPU(s), {n_rv * rf} reference + {args.noise_rows or n_rv * rf} noise frames")
        else:
            workload = ("BASELINE configs[1]: brute-force cosine search 200k query x 2M ref 512-d fp32 per GPU "
                        "+ candidates + TN localization (full hot path)")
        out = {
            "metric": "query-videos localized/sec @ 512-d SSCD",
            "value": total_videos / dt,
            "unit": "query-videos/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "fp32 results; int8 / fp16 MFMA pre-filters",
            "dtype_note": "every reported score is the exact fp32 fma chain (bit-identical to the all-fp32 "
                          "path); int8 and fp16 MFMA only pre-filter pairs, each with a rigorous error bound",
            "data": "synthetic" if args.data == "gaussian" else f"synthetic ({args.data})",
            "process_group": pg,
            "config": {
                "workload": workload,
                "query_videos_per_gpu": n_qv, "query_frames_per_gpu": n_qv * qf, "ref_frames": n_rv * rf,
                "dim": dim, "global_k": 1200 * n_qv_total, "candidates": res.n_candidates,
                "pairs_localized": res.n_localized, "matches": res.n_matches, "hits": res.n_hits,
                "score_normalisation_in_step": strong,
                "parallelism": f"query-sharded x{world}" if world > 1 else "single GPU",
            },
        }
        if args.full:
            steps = args.steps
            # Dominant kernel = the similarity kernel class with the most time on the engine's stream: the int8 panel
            # pre-filter (csrc/sim_i8p.hip), the fp16 one (csrc/sim_f16p.hip) or the exact fp32 kernel.  achieved =
            # algorithmic operations (2 * rows * refs * dim of its launches) / their HIP-event time.
            classes = {
                "i8": ("sim_i8p_kernel (panel-stationary int8 MFMA pre-filter on v_mfma_i32_16x16x64_i8: the kernel's own launches "
                       "-- the sparse batches of the search and the 1-NN passes of the score normalisation; the quantisation / "
                       "sorting of its query rows is reported under kernels as its preamble)", INT8_MFMA_PEAK_TOPS, "TOP/s"),
                "f16": ("sim_f16p_kernel (panel-stationary fp16 MFMA pre-filter; exact fp32 re-scoring of its candidates "
                        "follows)", FP16_MFMA_PEAK_TFLOPS, "TFLOP/s"),
                "sim": ("sim_thresh_kernel (fp32 MFMA similarity + fused threshold compaction)", FP32_MFMA_PEAK_TFLOPS, "TFLOP/s"),
            }
            # (configs[3]: the search index and the noise index of the score normalisation launch the same kernels)
            both = dict(prof)
            if nprof is not None:
                for c in classes:
                    for f in ("ms", "flops", "launches"):
                        both[f"{c}_{f}"] = prof.get(f"{c}_{f}", 0) + nprof.get(f"{c}_{f}", 0)
            dom = max(classes, key=lambda c: both.get(f"{c}_ms", 0.0))
            k_ms, k_flops, k_launches = both[f"{dom}_ms"], both[f"{dom}_flops"], both[f"{dom}_launches"]
            peak = classes[dom][1]
            achieved = (k_flops / 1e12) / (k_ms / 1e3) if k_ms > 0 else 0.0
            # HBM-side bytes per launch of the dominant kernel come from the committed PMC passes of the SAME kernel
            # (FETCH_SIZE / WRITE_SIZE cannot be sampled from inside the process): the newest profiles/r*_roofline.json names
            # the kernel, the commit it was measured at, the rocprofv3 files and the hash of the kernel's source file then --
            # compared with the file as it is now, so the line says whether the figure belongs to this very kernel
            traffic, traffic_src = None, None
            try:
                import glob
                import hashlib
                rpath = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_roofline.json")))[-1]
                with open(rpath) as fh:
                    rj = json.load(fh)
                if rj.get("kernel_class") == dom:
                    traffic = float(rj["hbm_bytes_per_launch"])
                    traffic_src = f"profiles/{os.path.basename(rpath)}, measured at commit {rj.get('commit', '?')}"
                    if rj.get("kernel_source"):
                        with open(os.path.join(ROOT, rj["kernel_source"]), "rb") as fh:
                            same = hashlib.sha256(fh.read()).hexdigest()[:16] == rj.get("kernel_source_sha256_16")
                        traffic_src += f"; {rj['kernel_source']} {'unchanged' if same else 'CHANGED'} since"
            except Exception:
                pass
            dpad_bytes = 8 * ((dim + 63) // 64 * 64)  # two packed fp32 rows per re-scored candidate
            cand = prof.get("candidates", 0)
            kernels = {
                "sim_i8p_kernel (int8 MFMA pre-filter, sparse batches)": {
                    "ms_per_step": prof.get("i8_ms", 0.0) / steps, "launches_per_step": prof.get("i8_launches", 0) / steps,
                    "achieved": _rate(prof.get("i8_flops", 0.0), prof.get("i8_ms", 0.0), 1e12),
                    "peak": INT8_MFMA_PEAK_TOPS, "unit": "TOP/s", "bound": "mfma"},
                "int8 launches' preamble (row thresholds / scales, sort of the launch's rows, quantisation of the panels)": {
                    "ms_per_step": prof.get("i8_prep_ms", 0.0) / steps, "launches_per_step": prof.get("i8_prep_launches", 0) / steps},
                "sim_f16p_kernel (fp16 MFMA pre-filter)": {
                    "ms_per_step": prof.get("f16_ms", 0.0) / steps, "launches_per_step": prof.get("f16_launches", 0) / steps,
                    "achieved": _rate(prof.get("f16_flops", 0.0), prof.get("f16_ms", 0.0), 1e12),
                    "peak": FP16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "bound": "mfma"},
                "sim_thresh_kernel (exact fp32 MFMA, dense early batches)": {
                    "ms_per_step": prof["sim_ms"] / steps, "achieved": _rate(prof["sim_flops"], prof["sim_ms"], 1e12),
                    "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "bound": "mfma"},
                "rescore_kernel (exact fp32 chain of the candidates)": {
                    "ms_per_step": prof.get("rescore_ms", 0.0) / steps,
                    # HBM/fabric side: one REFERENCE row per candidate (a random 2 KB read of the 4 GB image; the query rows
                    # of a segment are one 128-row panel and stay in L2).  l2_to_cu counts both rows.
                    "achieved": _rate(float(cand) * (dpad_bytes // 2) * steps, prof.get("rescore_ms", 0.0), 1e9),
                    "l2_to_cu_GBs": _rate(float(cand) * dpad_bytes * steps, prof.get("rescore_ms", 0.0), 1e9),
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "bound": "hbm / fabric gather",
                    "note": f"{cand} candidates of the last search x {dpad_bytes // 2} B reference row (+ as many query-row bytes from L2)"},
                "select_* (radix select + compaction of the re-thresholds)": {
                    "ms_per_step": prof.get("select_ms", 0.0) / steps, "launch_groups_per_step": prof.get("select_launches", 0) / steps},
                "final ordering of the kept hits (radix sorts)": {
                    "ms_per_step": prof.get("sort_ms", 0.0) / steps,
                    "achieved": _rate(prof.get("sort_flops", 0.0), prof.get("sort_ms", 0.0), 1e9), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "bound": "hbm", "note": "algorithmic bytes = 12 B per kept hit in; ~20 passes inside"},
                "pair_max (sort by pair + segmented max + rank sort)": {
                    "ms_per_step": pm_ms / steps, "achieved": _rate(pm_bytes, pm_ms, 1e9), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "bound": "hbm"},
                "tn_pair_kernel (Temporal Network, one pair per wavefront)": {
                    "ms_per_step": tn_ms / steps, "achieved": _rate(tn_bytes, tn_ms, 1e9), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "bound": "hbm by its bytes (instruction-issue-bound in practice: DESIGN.md 8.6)",
                    "note": "algorithmic bytes = 4 * dim * (Lq + Lr) per pair + boxes"},
            }
            if nprof is not None:
                kernels["score normalisation of the query set (1-NN vs the noise index: exact subset pass + pre-filter + re-scoring)"] = {
                    "ms_per_step": (nprof["sim_ms"] + nprof["f16_ms"] + nprof["i8_ms"] + nprof.get("i8_prep_ms", 0.0) + nprof["rescore_ms"]) / steps,
                    "int8_prefilter_ms_per_step": nprof["i8_ms"] / steps, "int8_preamble_ms_per_step": nprof.get("i8_prep_ms", 0.0) / steps,
                    "fp16_prefilter_ms_per_step": nprof["f16_ms"] / steps,
                    "achieved": _rate(nprof["i8_flops"] + nprof["f16_flops"], nprof["i8_ms"] + nprof["f16_ms"], 1e12),
                    "unit": "T(FL)OP/s of the pre-filter passes"}
            for v in kernels.values():
                if "achieved" in v and v.get("peak"):
                    v["frac"] = v["achieved"] / v["peak"]
            out.update({
                "result_digest": digest["result_digest"],
                "result_digest_parts": dict(digest["parts"], n_boxes=digest["n_boxes"], tie_on_cut=digest["tie_on_cut"],
                                            ties_dropped=digest["ties_dropped"],
                                            note="sha256 of (final radius | candidate table | localised segments): identical for "
                                                 "--gpus 1 and --gpus N runs of the same command line"),
                "roofline": {
                    "kernel": classes[dom][0],
                    "bound": "mfma",
                    "achieved": achieved,
                    "peak": peak,
                    "unit": classes[dom][2],
                    "frac": achieved / peak,
                    "traffic": traffic,
                    "traffic_unit": f"bytes/launch (PMC FETCH_SIZE x2 + WRITE_SIZE; {traffic_src})" if traffic else None,
                    "launches": k_launches,
                    "kernel_ms_per_step": k_ms / args.steps,
                    "prefilter_candidates_last_search": cand,
                },
                "kernels": kernels,
            })
        if world > 1 and args.full:
            # what the sharded search did in the last step on rank 0 (engine.DeviceMatcher.sharded_schedule_search): batches
            # searched, and -- with VSC_SHARD_DEBUG=1, which synchronises around every phase -- the seconds per phase.  In the
            # share-GPU debugging set-up t_gather / t_handover are host-staged gloo transfers and the GPU phases are the work
            # of ALL ranks interleaved on one device
            st = getattr(matcher, "last_shard_stats", None)
            if st:
                out["sharded_search"] = dict(mode=os.environ.get("VSC_SHARD_MODE", "cols"), share_gpu=share_gpu,
                                             **{k: (round(v, 4) if isinstance(v, float) else v) for k, v in st.items() if k != "phases"})
                # per phase of the last step, MAX over ranks: host wall ms, device ms between HIP events on the engine's
                # stream (no synchronisation added), calls, bytes handed to the collective
                out["sharded_search"]["phases_max_over_ranks"] = shard_phases
                out["sharded_search"]["phases_note"] = (
                    "gather_queries = all-gather of the score-normalised query rows; search = the rank's column slice of every "
                    "batch (library calls); count = per-batch all-reduce of the kept total (+ its host sync); events = exact "
                    "distributed (K+1)-th best by radix-select histograms + filter; handover = all-to-all of the kept hits to "
                    "the row owners; final_sort_and_cut = radix sort + distributed cut at K")
        if world == 1 and args.full:
            # the untimed legs must never cost the headline line: a failure in one of them is reported, not raised
            if not args.no_extra:
                try:
                    if strong:
                        del matcher, norm
                        torch.cuda.empty_cache()
                        out["extra"] = {"config2_shape": config2_shape_leg(args, torch, dev, dim)}
                        # non-Gaussian descriptors: the same shape on a cluster mixture
                        out["extra"]["clustered"] = distribution_leg(args, torch, dev, dim, "clusters")
                        # ... and on rows with a common direction + dominant coordinates, score-normalised (the class the int8
                        # bound is most sensitive to; its reference image is centred on the rows' mean)
                        out["extra"]["shifted"] = distribution_leg(args, torch, dev, dim, "offset", score_norm=True)
                    else:
                        out["extra"] = extra_legs(args, torch, dev, matcher, queries, n_qv, qf, n_rv, rf, dim)
                        ms_fresh = out["ms_per_step"] + out["extra"]["set_queries_ms"]
                        out["extra"]["value_with_fresh_query_set"] = n_qv / (ms_fresh / 1e3)
                        out["value_with_score_norm"] = n_qv / ((ms_fresh + out["extra"]["score_normalize_queries_ms"]) / 1e3)
                except Exception as exc:  # noqa: BLE001
                    out["extra_error"] = f"{type(exc).__name__}: {exc}"
            if not args.no_cpu_baseline:
                try:
                    out["cpu_baseline"] = cpu_baseline(args, strong)
                except Exception as exc:  # noqa: BLE001
                    out["cpu_baseline_error"] = f"{type(exc).__name__}: {exc}"
                try:
                    out["cpu_baseline_exact_port"] = cpu_baseline_exact_port(args, strong)
                except Exception as exc:  # noqa: BLE001
                    out["cpu_baseline_blas_error"] = f"{type(exc).__name__}: {exc}"
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
