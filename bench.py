#!/usr/bin/env python
"""bench.py — throughput of the MI355X BEVFusion hot path on synthetic nuScenes-shaped frames.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B | --global-batch G] [--full [--no-cpu-baseline] [--no-extras]]
                    [--spconv-dtype fp16|fp32|bf16] [--feat-dtype fp32|bf16] [--dump-outputs DIR] [--dry-run]

`--gpus N` with no launcher environment (WORLD_SIZE unset) re-executes this file under `torch.distributed.run` with N ranks on
127.0.0.1, one rank per GPU (RCCL); under a launcher it uses the ranks it was given.  `--dry-run` swaps the GPU work for a
stub on the host and the backend for gloo: the whole N>1 control flow (spawn, rendezvous, frame sharding, barriers,
max-over-ranks timing, the JSON line) runs in a container without GPUs (tests/test_bench_launch.py).

A "step" is ONE pass of the hot path over one batch of synthetic frames per GPU (--batch, default 8) at the C+L flagship
sizes, inputs already resident in HBM:
    camera branch : LiDAR -> per-camera depth images (depth raster), fused depth (x) context -> BEV pooling, and the API-level
                    bev_pool interval reduction of the [6*118*32*88, 80] frustum feature volume into the 360x360 BEV grid
                    (geometry + rank/sort/CSR plan cached: calibration is static at inference; uncached cost reported)
    LiDAR branch  : hard voxelization + mean of ~310k points (0.075 m voxels, 160k cap)
                    -> SparseEncoder (VoxelNet: 17 SubM + 4 strided sparse convs) -> [1, 256, 180, 180]
One process per GPU; for N>1 the driver launches this file under torch.distributed.run and ranks meet only in
barriers (the path shards by frame: no data-path collective, weak scaling).

Prints ONE JSON line on rank 0 with `roofline` for the dominant kernel (bev_pool scatter, HBM-bound).  A plain run only sets up,
warms up, times the K steps and prints the line; `--full` adds every secondary measurement after the timed region: the roofline
kernel solo, `cpu_baseline` (reference algorithms on the host cores, bounded sample), `extra`, `roofline_spconv` and the uncached
plan costs.  `--dump-outputs DIR` writes what the last timed step computed as .npy files.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec (6.29 TB/s measured copy ceiling)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--feat-dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--spconv-dtype", choices=["fp16", "fp32", "bf16"], default="fp16")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--batch", type=int, default=None,
                    help="frames per step per GPU (default 8: BASELINE.json's C+L inference config is quoted at batch 8 on one GPU; "
                         "--batch 1 = single-frame latency)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="fixed number of frames per step for the WHOLE job, split over the ranks with sharding.frames_for_rank "
                         "(strong scaling); default 0 = --batch frames on every GPU (weak scaling)")
    ap.add_argument("--overlap", choices=["auto", "ahead", "chain", "pipeline", "voxel", "head", "lidar", "none"], default="auto",
                    help="auto: ahead from 2 frames per step (round 6; 1.39 / 1.96 ms against 1.52 / 2.06 at 2 / 3 frames), voxel for a single frame (a latency figure).  ahead: software pipeline ACROSS steps over two alternating "
                         "buffer sets — the voxelizer + rulebook chain of batch t+1 run during step t beside the camera stages and the "
                         "convolutions of batch t; every step still pays one head and one tail and ends with batch t complete (one box, two "
                         "pairs, 8 frames: ahead 4.43 / 4.46, lidar 4.61 / 4.64 ms).  lidar (default of round 5): the whole LiDAR branch of "
                         "THIS batch beside the camera stages (round 5, one box, two pairs, 8 frames: "
                         "lidar 4.72 / 4.73, chain 4.81 / 4.85, head 4.83 / 4.83, voxel 4.84 / 4.85 ms; one frame: voxel 0.94, chain 1.16). "
                         "With lidar the camera kernels share the machine with the LiDAR branch, so roofline.kernel_ms is the bev_pool kernel "
                         "measured SOLO right after the timed region and kernel_ms_in_step the launch inside the step.  "
                         "chain: the voxelizer (own HIP graph, second stream) beside the depth raster / fused pooling, the "
                         "encoder's rulebook chain (own graph, same second stream) beside bev_pool — a pure HBM stream without LDS or MFMA "
                         "use, the partner a latency-bound integer chain wants —, then the 21 convolutions + dense tail ALONE after the "
                         "join; roofline.kernel_ms is then the bev_pool kernel measured SOLO after the timed region (kernel_ms_in_step: "
                         "with the chain beside it); voxel (default of round 4, see below); none: camera stages, then the whole LiDAR branch, back to back; pipeline: the stages of the two "
                         "independent branches interleaved so that each HBM-bound camera kernel has at most a light partner: bev_pool "
                         "runs first with only the voxelizer beside it (second HIP stream), the rulebook chain "
                         "(SparseEncoder.prepare_geometry) starts when bev_pool has finished and runs beside the depth raster and the "
                         "fused pooling, the convolutions follow after the join and run alone (measured at the end of round 3: 5.51-5.52 against 5.55 ms — "
                         "even the voxelizer alone costs bev_pool 24 %%, 1.27 against 1.03 ms; not a gain); voxel: only the voxelizer (22 "
                         "short dependent launches, 0.3 ms) runs on a second HIP stream beside the depth raster / fused pooling stages — it is "
                         "done long before bev_pool starts, whose roofline figure stays clean — and the encoder follows after the join (round 3: 5.34-5.38 "
                         "against 5.42-5.47 ms: the raster and the fused pooling pay 0.17 ms for the 0.3 ms hidden; round 4, with the column "
                         "pooling kernels: 4.93-5.00 against 5.06 ms per 8 frames, 1.07 against 1.15 ms on one frame, A/B on one box: the default); "
                         "head: the LiDAR branch's head — "
                         "voxelization + the whole rulebook chain (SparseEncoder.prepare_geometry) — runs on a second HIP stream beside the "
                         "camera stages and the convolutions follow after the join (round 3: 5.23-5.33 against 5.42-5.55 ms per 8-frame step — the 21 "
                         "convolutions then run alone in 2.87 ms — but the camera kernels pay 0.66 ms of it and bev_pool drops from 0.64 to "
                         "0.42 of the HBM peak: the default keeps the branches apart and that figure clean); "
                         "lidar: the WHOLE LiDAR branch (one HIP graph) runs on a second stream beside the camera stages, which is how the "
                         "two independent branches of the model can be scheduled; stage times then overlap and the bev_pool roofline figure "
                         "is measured WITH that concurrency")
    ap.add_argument("--amp", action="store_true",
                    help="--mode train-step: the reference's DEFAULT training arithmetic (configs/default.yaml:20-22 fp16 -> "
                         "Fp16OptimizerHook, apis/train.py:75-85): sparse convolutions under torch.autocast(float16) "
                         "(functional.py:24 custom_fwd(cast_inputs=torch.half)), fp32 master weights, dynamic loss scaling "
                         "(GradScaler, growth_interval 2000).  Without it the step runs in fp32 throughout.")
    ap.add_argument("--voxel-order", choices=["key", "first"], default="key",
                    help="row order of the voxelizer's output: key = ascending linear cell index (level 1 of the encoder then runs on the "
                         "staged-rows kernels with sorted-key neighbour search; the dense BEV output is identical), first = the "
                         "reference's first-appearance numbering (hash index + gather kernels at level 1)")
    ap.add_argument("--no-graph", action="store_true", help="launch the LiDAR branch kernel by kernel instead of replaying a HIP graph")
    ap.add_argument("--mode", choices=["infer", "train-step"], default="infer",
                    help="infer (default): the inference hot path of BASELINE configs[3]; train-step: forward + backward + optimizer "
                         "step of the same path in fp32 (BASELINE configs[4]: 4 frames per GPU unless --batch / --global-batch says "
                         "otherwise, gradients all-reduced over RCCL when --gpus > 1)")
    ap.add_argument("--train-inputs", choices=["augmented", "static"], default="augmented",
                    help="--mode train-step: augmented (default) = what a training step of the reference pays — per-sample image augmentation "
                         "(resize 0.38-0.55, rotate +-5.4 deg, flip) and LiDAR augmentation (rotate +-45 deg, scale 0.9-1.1, translate 0.5 m) drawn "
                         "per step, frustum geometry + pooling plan + column plan rebuilt INSIDE the timed step, point clouds rotating through a "
                         "pool; static = round 5's protocol (one test-time calibration, plan built once outside the timed loop, the same clouds)")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full, infer mode, one rank: skip the secondary measurements of `extra` (bev_pool on bf16 features = BASELINE "
                         "configs[1], the single-frame step, the product step without the double-counted API kernel, 5 steps of "
                         "--mode train-step --amp at 4 frames = configs[4]); they run AFTER the timed region and add ~20 s")
    ap.add_argument("--full", action="store_true",
                    help="infer mode: besides the timed steps, run every secondary measurement — the CPU baseline and `extra` (each "
                         "unless its --no-* flag is given), the per-layer convolution profile with its GEMM yardstick (roofline_spconv), "
                         "the roofline kernel solo after the timed region, the uncached plan / geometry costs and the eager LiDAR "
                         "sub-timings.  Without it a run sets up, warms up, times --steps steps and prints the line; its roofline "
                         "figure is then the bev_pool launch inside the timed steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0) as DIR/<name>.npy in float32 / "
                         "float64: whole arrays up to 2^21 elements, larger ones as a fixed seeded sample of 2^21 elements (sorted "
                         "flat indices drawn with seed 0), at most 64 MB in all.  Inputs are seeded: the same arguments give the "
                         "same inputs on every run")
    ap.add_argument("--cpu-baseline-worker", default=None, help=argparse.SUPPRESS)   # internal: child process of cpu_baseline()
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU: a host stub stands in for the hot path and gloo for RCCL, everything else (launch, sharding, "
                         "barriers, timing, JSON) is the real code path")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def respawn_under_launcher(args):
    """`python bench.py --gpus N` typed by hand: become N ranks.  (The driver launches torch.distributed.run itself; then
    WORLD_SIZE is set and this is skipped.)  Mirrors the reference's `torchpack dist-run -np N` (tools/train.py:20-29)."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def dry_run(args, rank, world, frame_ids):
    """The control flow of main() around a host stub: each rank 'processes' its frames (a seeded reduction per frame id),
    ranks meet in the barriers only, rank 0 prints the JSON line.  No GPU, gloo instead of RCCL."""
    import torch.distributed as dist

    from bevfusion_amd.sharding import barrier, max_over_ranks, sum_over_ranks

    def step():
        acc = 0.0
        for f in frame_ids:
            g = torch.Generator().manual_seed(1000 + f)
            acc += float(torch.randn(4096, generator=g).square().sum())
        return acc

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    checksum = 0.0
    for _ in range(args.steps):
        checksum = step()
    barrier()
    elapsed_local = time.perf_counter() - t0
    elapsed = max_over_ranks(elapsed_local)
    frames_per_step = int(sum_over_ranks(len(frame_ids)))
    total_checksum = sum_over_ranks(checksum)
    per_rank = [None] * world
    backend_ranks = int(sum_over_ranks(1))      # world size as an all-reduce of ones sees it ("rccl_ranks" of the GPU run)
    mine = dict(rank=rank, frames=list(frame_ids), ms_per_step=elapsed_local / args.steps * 1e3, cpu_binding=args.cpu_binding)
    if world > 1:
        dist.all_gather_object(per_rank, mine)
    else:
        per_rank = [mine]
    if rank == 0:
        print(json.dumps({
            "metric": "DRY RUN (host stub, no GPU work): launch / sharding / timing control flow of bench.py",
            "value": frames_per_step * args.steps / elapsed, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong" if args.global_batch else "weak", "vs_baseline": None, "dtype": "none", "data": "synthetic",
            "config": {"workload": "dry-run stub", "frames_per_step": frames_per_step, "backend": "gloo",
                       "world_size": world, "rccl_ranks": backend_ranks, "per_rank": per_rank, "checksum": total_checksum},
            "dry_run": True}), flush=True)


def wrap_for_gradient_allreduce(module, world, device=None):
    """The ONE collective of the path (apis/train.py:48-53): gradients are all-reduced by DistributedDataParallel over
    torch.distributed ("nccl" = RCCL over xGMI on the GPUs, gloo in --dry-run); a single rank trains the bare module."""
    if world <= 1:
        return module
    if device is not None and device.type == "cuda":
        return torch.nn.parallel.DistributedDataParallel(module, device_ids=[device.index])
    return torch.nn.parallel.DistributedDataParallel(module)


def dry_run_train(args, rank, world, frame_ids):
    """`--mode train-step --dry-run`: the DDP wiring of train_step() around a host stub of the trainable part (a small MLP
    standing in for the SparseEncoder), gloo instead of RCCL: per-rank data (seeded by frame id), the SAME initial weights on
    every rank, backward through DistributedDataParallel, clip_grad_norm + AdamW.  Reported: whether the per-rank inputs differ,
    whether the gradients and the updated weights agree on all ranks after the all-reduce, and that they equal the mean of the
    per-rank gradients computed without DDP."""
    import torch.distributed as dist

    from bevfusion_amd.sharding import barrier, max_over_ranks, sum_over_ranks

    torch.manual_seed(0)                                   # same initial weights everywhere (as make_encoder does)
    stub = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8))
    solo = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.ReLU(), torch.nn.Linear(32, 8))
    solo.load_state_dict(stub.state_dict())
    model = wrap_for_gradient_allreduce(stub, world)
    opt = torch.optim.AdamW(stub.parameters(), lr=2e-4, weight_decay=0.01)

    def batch():
        xs = [torch.randn(16, 64, generator=torch.Generator().manual_seed(1000 + f)) for f in frame_ids]
        return torch.cat(xs, 0) if xs else torch.zeros(0, 64)

    x = batch()
    data_sum = float(x.double().sum())
    # reference: this rank's own gradient without DDP, averaged over the ranks by hand
    solo(x).square().mean().backward()
    own = torch.cat([p.grad.reshape(-1) for p in solo.parameters()])
    mean_of_own = own.clone()
    if world > 1:
        dist.all_reduce(mean_of_own)
        mean_of_own /= world

    def step():
        model(x).square().mean().backward()
        g = torch.cat([p.grad.reshape(-1) for p in stub.parameters()]).clone()
        torch.nn.utils.clip_grad_norm_(stub.parameters(), 35.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        return g

    first_grad = step()
    for _ in range(max(0, args.warmup - 1)):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed_local = time.perf_counter() - t0
    elapsed = max_over_ranks(elapsed_local)
    frames_per_step = int(sum_over_ranks(len(frame_ids)))
    weights = torch.cat([p.detach().reshape(-1) for p in stub.parameters()])
    backend_ranks = int(sum_over_ranks(1))
    info = dict(rank=rank, frames=list(frame_ids), cpu_binding=args.cpu_binding, data_sum=data_sum, grad_sum=float(first_grad.double().sum()),
                grad_vs_mean_of_own=float((first_grad - mean_of_own).abs().max()), weight_sum=float(weights.double().sum()))
    per_rank = [None] * world
    if world > 1:
        dist.all_gather_object(per_rank, info)
    else:
        per_rank = [info]
    if rank == 0:
        print(json.dumps({
            "metric": "DRY RUN (host stub, no GPU work): DistributedDataParallel wiring of --mode train-step",
            "value": frames_per_step * args.steps / elapsed, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong" if args.global_batch else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "dry-run stub of the training step", "frames_per_step": frames_per_step, "backend": "gloo",
                       "world_size": world, "rccl_ranks": backend_ranks, "per_rank": per_rank,
                       "ddp": world > 1,
                       "inputs_differ_across_ranks": len({r["data_sum"] for r in per_rank}) == world,
                       "gradients_agree_across_ranks": max(r["grad_sum"] for r in per_rank) - min(r["grad_sum"] for r in per_rank) == 0.0,
                       "weights_agree_across_ranks": max(r["weight_sum"] for r in per_rank) - min(r["weight_sum"] for r in per_rank) == 0.0,
                       "max_abs_grad_minus_mean_of_per_rank_grads": max(r["grad_vs_mean_of_own"] for r in per_rank)},
            "dry_run": True}), flush=True)


LINE_LIMIT = 4096   # bytes of the ONE JSON line on stdout; tests/test_bench_launch.py hard-fails above 8192


def _r(v, sig=5):
    """floats to `sig` significant digits (the line is for parsing, the side file keeps full precision)"""
    if isinstance(v, float):
        v = float(f"{v:.{sig}g}")
        return int(v) if abs(v) >= 1e6 and v == int(v) else v
    if isinstance(v, dict):
        return {k: _r(x, sig) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_r(x, sig) for x in v]
    return v


def _backend_name():
    """'nccl (= RCCL)' on a multi-GPU node; 'gloo' under BEVAMD_BENCH_SHARED_GPU (tests: several ranks on one device)"""
    import torch.distributed as dist

    b = dist.get_backend() if dist.is_available() and dist.is_initialized() else "none"
    return "nccl (= RCCL)" if b == "nccl" else b


def compact_line(res, side_file=None):
    """The ONE line the driver parses, from the full result `res` (which goes to the side file): the contract keys, the
    roofline of the dominant kernel, the CPU baseline's figures, the secondary measurements as bare numbers.  No per-layer tables,
    no thread sweeps, no prose notes (round 4's 23-KB line left BENCH_r04.parsed null).  Pure function: tested on the CPU."""
    cfg = res.get("config") or {}
    out = {k: res.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                   "scaling", "vs_baseline", "dtype", "data")}
    per_rank = cfg.get("per_rank") or []
    ms = [r["ms_per_step"] for r in per_rank if isinstance(r, dict) and "ms_per_step" in r]
    out["config"] = {k: cfg[k] for k in ("workload", "frames_per_step", "frames_per_step_per_gpu", "rccl_ranks", "stage_ms", "overlap",
                                         "inputs", "hip_graph", "gradient_allreduce", "plan_ms", "runs_per_column", "fused_kernel", "encoder_path") if k in cfg}
    if ms:
        out["config"]["per_rank_ms_per_step"] = {"min": min(ms), "max": max(ms)}
    rf = res.get("roofline")
    if rf:
        out["roofline"] = {k: rf.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic",
                                                  "algorithmic_bytes_per_launch", "kernel_ms", "kernel_ms_back_to_back", "rocprof_kernel_us", "kernel_ms_in_step", "frac_in_step", "measured") if k in rf}
    else:
        out["roofline"] = None
    cb = res.get("cpu_baseline")
    if cb:
        keep = {k: cb.get(k) for k in ("value", "unit", "cores", "kind", "seconds_per_frame", "bev_pool_quickcumsum_ms",
                                       "bev_pool_quickcumsum_threads", "voxelize_restated_ms", "voxelize_reference_cubic_ms")
                if k in cb}
        if "bev_pool_quickcumsum_spread" in cb:
            keep["spread"] = cb["bev_pool_quickcumsum_spread"]
        if "encoder_one_rulebook_per_stage_s" in cb:
            keep["encoder_s"] = cb["encoder_one_rulebook_per_stage_s"]
        keep["sample"] = cb.get("sample_short") or (cb.get("sample") or "")[:200]
        out["cpu_baseline"] = keep
    else:
        out["cpu_baseline"] = None
    ex = res.get("extra")
    if ex:
        e = {}
        g = lambda name, key: (ex.get(name) or {}).get(key)
        e["product_step_ms"] = g("product_step", "ms_per_step")
        e["product_frames_per_s"] = g("product_step", "frames_per_s")
        e["batch1_ms"] = g("batch1_step", "ms_per_step")
        e["batch1_lidar_branch_ms"] = g("batch1_step", "lidar_branch_ms")
        e["lidar_branch_alone_ms"] = g("lidar_branch_alone", "ms")
        e["convolutions_alone_ms"] = g("lidar_branch_alone", "convolutions_alone_ms")
        e["unpipelined_step_ms"] = g("unpipelined_step", "ms_per_step")
        e["ahead_output_equals_eager"] = ex.get("ahead_output_equals_eager")
        e["varied_rig_step_ms"] = g("varied_rig_step", "ms_per_step")
        e["alone_step_ms"] = g("bev_pool_alone_step", "ms_per_step")
        e["alone_frac_in_step"] = g("bev_pool_alone_step", "frac_in_step")
        e["bf16_frac"] = g("bev_pool_bf16_features", "frac")
        e["bf16_kernel_ms"] = g("bev_pool_bf16_features", "kernel_ms")
        e["train_amp_ms"] = g("train_step_amp", "ms_per_step")
        e["train_amp_frames"] = g("train_step_amp", "frames")
        e["train_amp_bev_pool_bwd_frac"] = g("train_step_amp", "bev_pool_bwd_frac")
        e["train_amp_plan_ms"] = g("train_step_amp", "plan_ms")
        e["train_amp_runs_per_column"] = g("train_step_amp", "runs_per_column")
        e["train_amp_fused_kernel"] = g("train_step_amp", "fused_kernel")
        e["fused_pool_alone_ms"] = g("fused_pool", "alone_ms")
        e["fused_pool_rigged_ms"] = g("fused_pool", "rigged_ms")
        e["kernel_nodes"] = (ex.get("lidar_graph") or {}).get("kernel_nodes")
        for name in ("batch1_step", "train_step_amp", "fused_pool"):
            if (ex.get(name) or {}).get("error"):
                e[name + "_error"] = ex[name]["error"][:120]
        out["extra"] = {k: v for k, v in e.items() if v is not None}
    rs = res.get("roofline_spconv")
    if rs:
        out["roofline_spconv"] = {k: rs.get(k) for k in ("total_us", "total_gflop", "tflops", "frac_mfma_peak", "n_layers", "dense_tap_tflops", "gemm_yardstick_tflops",
                                                          "dense_tap_frac_of_gemm_yardstick") if k in rs}
    bx = res.get("box")
    if bx:
        out["box"] = {k: bx[k] for k in ("gpu_unique_id", "pci", "sclk", "mclk") if k in bx}
    if side_file:
        out["full_result"] = side_file
    out = _r(out)
    line = json.dumps(out, separators=(",", ":"))
    if len(line) > LINE_LIMIT:           # never again an unparseable line: shed the optional parts, keep the contract
        for k in ("roofline_spconv", "extra"):
            out.pop(k, None)
            line = json.dumps(out, separators=(",", ":"))
            if len(line) <= LINE_LIMIT:
                break
    return line


def emit(res):
    """Rank 0: full result -> profiles/bench_last_full.json (and gpurun_out/ when it exists, so that it travels back from a gpurun
    visit), compact line -> stdout."""
    side = None
    for d in ("profiles", "gpurun_out"):
        p = os.path.join(ROOT, d)
        if os.path.isdir(p):
            try:
                with open(os.path.join(p, "bench_last_full.json"), "w") as fh:
                    json.dump(res, fh, indent=1)
                side = side or os.path.join(d, "bench_last_full.json")
            except OSError:
                pass
    print(compact_line(res, side), flush=True)


DUMP_ELEMS = 1 << 21   # per array: 8 MB in float32; the step's largest outputs (330 MB each at 8 frames) are sampled to this


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each tensor of {name: tensor} -> out_dir/<name>.npy, floating point as float32, integers as float64.
    A tensor of more than DUMP_ELEMS elements is reduced ON THE DEVICE to the elements at DUMP_ELEMS sorted flat indices drawn
    with a fixed seed from its element count: the same positions on every run, so two builds compare element for element."""
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        if flat.numel() > DUMP_ELEMS:
            idx = torch.randint(flat.numel(), (DUMP_ELEMS,), generator=torch.Generator().manual_seed(0)).sort().values
            flat = flat[idx.to(flat.device)]
        flat = flat.float() if flat.is_floating_point() else flat.double()
        np.save(os.path.join(out_dir, name + ".npy"), flat.cpu().numpy())


def box_info(dev_index=0):
    """Which box and which clocks a line was measured on (0.885 / 0.954 / 1.009 ms for one kernel on three
    boxes could not be attributed): hostname, device name, the DPM levels sysfs marks current for the shader and memory clocks
    (read right after the timed region, i.e. under load) and the device's compute-unit count.  Best effort: never raises."""
    import glob
    import socket

    info = {"hostname": socket.gethostname()}
    try:
        p = torch.cuda.get_device_properties(dev_index)
        info.update(device=p.name, gcn_arch=getattr(p, "gcnArchName", None), compute_units=p.multi_processor_count,
                    hbm_gb=round(p.total_memory / 2 ** 30, 1))
    except Exception:
        pass
    # the sysfs node of THIS device (a node shows all its GPUs' cards; only one is visible to the process): by PCI address
    node = None
    try:
        p = torch.cuda.get_device_properties(dev_index)
        bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
        if os.path.isdir(f"/sys/bus/pci/devices/{bdf}"):
            node = f"/sys/bus/pci/devices/{bdf}"
            info["pci"] = bdf
    except Exception:
        pass
    nodes = [node] if node else [os.path.dirname(c) for c in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))]
    for key, fname in (("sclk", "pp_dpm_sclk"), ("mclk", "pp_dpm_mclk"), ("fclk", "pp_dpm_fclk")):
        cur = []
        for c in nodes:
            try:
                with open(os.path.join(c, fname)) as fh:
                    cur += [ln.split(":")[1].strip().rstrip("*").strip() for ln in fh if ln.rstrip().endswith("*")]
            except OSError:
                pass
        if cur:
            info[key] = cur if len(set(cur)) > 1 else cur[0]
    if node:
        try:
            info["gpu_unique_id"] = open(os.path.join(node, "unique_id")).read().strip()
        except OSError:
            pass
    return info


class quiet_gc:
    """The timed region without the cyclic garbage collector (what `timeit` does): a full collection over the ~10^6 objects of a
    process that has imported torch and built the models is a 100-ms host stall — seen as ONE 119-ms encoder forward among
    5.8-ms ones in the 7th step of `--mode train-step --amp`, whose forward is paced by the host (per_step_ms in its JSON)."""

    def __enter__(self):
        import gc

        self.was = gc.isenabled()
        gc.collect()
        gc.disable()

    def __exit__(self, *exc):
        import gc

        if self.was:
            gc.enable()
        return False


def new_graph():
    """A CUDAGraph that keeps its hipGraph_t, so that its nodes can be counted (torch >= 2.8); plain otherwise."""
    try:
        return torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        return torch.cuda.CUDAGraph()


def graph_node_count(graph):
    """{'nodes': all nodes, 'kernel_nodes': kernel launches} of a captured graph through hipGraphGetNodes / hipGraphNodeGetType,
    None when the runtime or this torch build does not expose the graph."""
    import ctypes

    try:
        raw = graph.raw_cuda_graph()
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_size_t(0)
        if hip.hipGraphGetNodes(ctypes.c_void_p(raw), None, ctypes.byref(n)) != 0:
            return None
        nodes = (ctypes.c_void_p * max(n.value, 1))()
        if hip.hipGraphGetNodes(ctypes.c_void_p(raw), nodes, ctypes.byref(n)) != 0:
            return None
        kernels = 0
        for i in range(n.value):
            kind = ctypes.c_int(-1)
            if hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(kind)) == 0 and kind.value == 0:   # hipGraphNodeTypeKernel
                kernels += 1
        return dict(nodes=int(n.value), kernel_nodes=kernels)
    except Exception:
        return None


def make_encoder(cfg, dev, dtype):
    from bevfusion_amd.sparse_encoder import SparseEncoder

    torch.manual_seed(0)
    enc = SparseEncoder(5, list(cfg["sparse_shape"]), order=["conv", "norm", "act"], output_channels=128,
                        encoder_channels=[[16, 16, 32], [32, 32, 64], [64, 64, 128], [128, 128]],
                        encoder_paddings=[[0, 0, 1], [0, 0, 1], [0, 0, [1, 1, 0]], [0, 0]], block_type="basicblock")
    return enc.to(dev).to(dtype).eval()


# ---------------------------------------------------------------------------------------------------------
# CPU baseline (rank 0, N=1 only): reference algorithms on the host cores, bounded to ~20 s
# ---------------------------------------------------------------------------------------------------------
def cpu_bev_pool_quickcumsum(coords_kept, feats_kept, B, D, H, W):
    """QuickCumsum (bev_pool.py:8-34) + prologue (bev_pool.py:83-93) with PyTorch CPU ops, all cores."""
    x = torch.from_numpy(feats_kept)
    coords = torch.from_numpy(coords_kept)
    t0 = time.perf_counter()
    ranks = coords[:, 0] * (W * D * B) + coords[:, 1] * (D * B) + coords[:, 2] * B + coords[:, 3]
    indices = ranks.argsort()
    xs, cs, rs = x[indices], coords[indices], ranks[indices]
    xc = xs.cumsum(0)
    kept = torch.ones(xc.shape[0], dtype=torch.bool)
    kept[:-1] = rs[1:] != rs[:-1]
    xk, ck = xc[kept], cs[kept]
    xk = torch.cat((xk[:1], xk[1:] - xk[:-1]))
    out = torch.zeros((B, D, H, W, x.shape[1]), dtype=x.dtype)
    out[ck[:, 3], ck[:, 2], ck[:, 0], ck[:, 1]] = xk
    out = out.permute(0, 4, 1, 2, 3).contiguous()
    return time.perf_counter() - t0


def cpu_sparse_encoder_reference(coords_np, cfg):
    """Rulebook + convolution of every SparseEncoder layer with the REFERENCE's CPU functors
    (oracle/_ref/sparse_conv_ext: indice_cpu.cc, reordering_cpu.cc, spconv_ops.h).  One pass with one rulebook per distinct
    geometry; every rulebook is timed on its own so that the reference's recompute pattern (SparseBasicBlock passes
    indice_key=None: 16 of the 17 SubM rulebooks are rebuilt) is the same measured terms re-added.
    Returns dict(seconds_once, seconds_recompute, rulebook_s=[...]) or None if the reference build did not travel."""
    try:
        from oracle import ref_build

        ext = ref_build.load_ref("sparse_conv_ext")
    except Exception:
        return None
    from oracle import get_conv_output_size

    ind = torch.from_numpy(coords_np.astype(np.int32))
    shape = list(cfg["sparse_shape"])
    plan = [  # (cin, cout, n_convs, subm) then the strided conv leaving the stage
        ("subm", 5, 16, 1), ("subm", 16, 16, 4), ("conv", 16, 32, (3, 3, 3), (2, 2, 2), (1, 1, 1)),
        ("subm", 32, 32, 4), ("conv", 32, 64, (3, 3, 3), (2, 2, 2), (1, 1, 1)),
        ("subm", 64, 64, 4), ("conv", 64, 128, (3, 3, 3), (2, 2, 2), (1, 1, 0)),
        ("subm", 128, 128, 4), ("conv", 128, 128, (1, 1, 3), (1, 1, 2), (0, 0, 0)),
    ]
    t0 = time.perf_counter()
    subm_rb, t_rb, extra, rulebook_s = None, 0.0, 0.0, []
    for item in plan:
        if item[0] == "subm":
            _, cin, cout, reps = item
            if subm_rb is None:
                t1 = time.perf_counter()
                subm_rb = ext.get_indice_pairs_3d(ind, 1, shape, shape, [3, 3, 3], [1, 1, 1], [1, 1, 1], [1, 1, 1],
                                                  [0, 0, 0], 1, 0)
                t_rb = time.perf_counter() - t1
                rulebook_s.append(t_rb)
                first_of_level = True
            else:
                first_of_level = False
            # reference pattern: conv_input (indice_key "subm1") builds the level-1 rulebook once; every convolution inside a
            # SparseBasicBlock rebuilds it (sparse_encoder.py:140,194-199)
            extra += t_rb * (reps if not first_of_level or cin != 5 else 0)
            f = torch.randn(ind.shape[0], cin)
            w = torch.randn(3, 3, 3, cin, cout)
            for _ in range(reps):
                ext.indice_conv_fp32(f, w, subm_rb[1], subm_rb[2], ind.shape[0], 0, 1)
        else:
            _, cin, cout, ks, st, pd = item
            oshape = get_conv_output_size(shape, list(ks), list(st), list(pd), [1, 1, 1])
            t1 = time.perf_counter()
            rb = ext.get_indice_pairs_3d(ind, 1, oshape, shape, list(ks), list(st), list(pd), [1, 1, 1], [0, 0, 0], 0, 0)
            rulebook_s.append(time.perf_counter() - t1)
            f = torch.randn(ind.shape[0], cin)
            w = torch.randn(*ks, cin, cout)
            ext.indice_conv_fp32(f, w, rb[1], rb[2], rb[0].shape[0], 0, 0)
            ind, shape, subm_rb = rb[0].contiguous(), oshape, None
    once = time.perf_counter() - t0
    # per level the single pass built the SubM rulebook once; the reference builds it for every block convolution:
    # level 1: conv_input builds it (kept), 4 block convs rebuild -> +4; levels 2-4: 4 block convs -> 4 builds, one is in `once` -> +3
    return dict(seconds_once=once, seconds_recompute=once + extra - sum(rulebook_s[i] for i in (2, 4, 6) if i < len(rulebook_s)),
                rulebook_s=rulebook_s)


def _median_time(fn, runs=5, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def cpu_baseline(inp, pts, cfg, B, D, H, W):
    """BASELINE.md §3 protocol on the host cores of the GPU box, rank 0 / N=1 only, ONE frame (the first of the batch), in a CHILD
    process: the OpenMP runtime of a process binds its threads once, at start-up, so the thread placement the measurement needs
    (OMP_PLACES=cores, OMP_PROC_BIND=close: thread i on physical core i, no migration, no SMT sharing) cannot be switched on in a
    process that has already run torch — and the child is free of the HIP runtime's helper threads.  Rounds 2-3 measured
    QuickCumsum in-process with unbound threads: 4.6-17.8 s run to run.  The inputs travel through /dev/shm."""
    import subprocess
    import tempfile

    per_frame = inp["geom"].shape[0]          # `inp` holds ONE frame (geometry and features of frame 0)
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(prefix="bevamd_cpu_", dir=shm) as tmp:
        np.save(os.path.join(tmp, "geom.npy"), inp["geom"][:per_frame])
        np.save(os.path.join(tmp, "feats.npy"), inp["feats"][:per_frame])
        np.save(os.path.join(tmp, "pts.npy"), pts)
        with open(os.path.join(tmp, "meta.json"), "w") as fh:
            json.dump(dict(origin=[float(v) for v in inp["origin"]], dx=[float(v) for v in inp["dx"]],
                           nx=[int(v) for v in inp["nx"]], D=D, H=H, W=W), fh)
        try:
            import psutil

            physical = psutil.cpu_count(logical=False) or (os.cpu_count() or 2) // 2
        except Exception:
            physical = max(1, (os.cpu_count() or 2) // 2)
        try:
            physical = max(1, min(physical, len(os.sched_getaffinity(0))))
        except (AttributeError, OSError):
            pass
        env = dict(os.environ, OMP_PLACES="cores", OMP_PROC_BIND="close", OMP_NUM_THREADS=str(physical), MKL_NUM_THREADS=str(physical),
                   HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", BEVAMD_CPU_PHYSICAL=str(physical))
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", tmp], capture_output=True, text=True,
                           env=env, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return dict(value=None, unit="frames/s", cores=physical, kind="port", sample="cpu baseline worker failed: " + r.stderr[-500:])
    return json.loads(lines[-1])


def cpu_baseline_worker(tmp):
    """Child of cpu_baseline(): threads bound by the environment it was started with.  Prints ONE JSON object."""
    import oracle  # checker / baseline only

    cfg = __import__("bevfusion_amd.synth", fromlist=["CL_CONFIG"]).CL_CONFIG
    meta = json.load(open(os.path.join(tmp, "meta.json")))
    geom, feats, pts = (np.load(os.path.join(tmp, f + ".npy")) for f in ("geom", "feats", "pts"))
    D, H, W = meta["D"], meta["H"], meta["W"]
    origin, dx, nx = (np.asarray(meta[k], dtype=t) for k, t in (("origin", np.float32), ("dx", np.float32), ("nx", np.int64)))
    physical = int(os.environ.get("BEVAMD_CPU_PHYSICAL", torch.get_num_threads()))
    n_cam = cfg["num_cameras"]
    coords, kept = oracle.bev_cell_index(geom, 1, origin, dx, nx)
    ck, fk = coords[kept], feats[kept]
    # thread-count sweep on ONE camera's rows (a sixth of the frame: the sweep stays short), 1 warm-up + 3 runs each;
    # torch's CPU kernels of this pipeline (argsort, gather, cumsum over dim 0, index_put) stop scaling long before 64 cores
    cam_rows = np.flatnonzero(kept) < geom.shape[0] // n_cam
    ck1, fk1 = np.ascontiguousarray(ck[cam_rows]), np.ascontiguousarray(fk[cam_rows])
    sweep = []
    for t in sorted({min(t, physical) for t in (4, 8, 16, 32, 64, physical)}):
        torch.set_num_threads(t)
        med, runs = _median_time(lambda: cpu_bev_pool_quickcumsum(ck1, fk1, 1, D, H, W), runs=3, warmup=1)
        sweep.append(dict(threads=t, median_ms=med * 1e3, runs_ms=[r * 1e3 for r in runs]))
    best = min(sweep, key=lambda e: e["median_ms"])
    threads = best["threads"]
    torch.set_num_threads(threads)
    t_bev, bev_runs = _median_time(lambda: cpu_bev_pool_quickcumsum(ck, fk, 1, D, H, W), runs=5, warmup=2)
    n_int = int(np.unique(oracle.bev_pool_ranks(ck, 1, D, H, W)).shape[0])
    bev_bytes = ck.shape[0] * fk.shape[1] * 4 + n_int * 24 + D * H * W * fk.shape[1] * 4
    torch.set_num_threads(physical)
    # voxelization (a) restated serial algorithm on the real 1440x1440x40 grid (the reference's own CPU code is memory-unsafe
    # there), (b) the reference's hard_voxelize_cpu on a CUBIC grid of equal cell count, where it is safe
    def restated():
        v, c, n = oracle.hard_voxelize(pts, cfg["voxel_size"], cfg["point_cloud_range"], cfg["max_num_points"], cfg["max_voxels"][1])
        oracle.voxel_mean(v, n)
        return c

    t_vox, _ = _median_time(restated)
    c = restated()
    t_vox_ref = None
    try:
        from oracle import ref_build

        vext = ref_build.load_ref("voxel_layer")
        r = cfg["point_cloud_range"]
        side = int(round((1440 * 1440 * 40) ** (1.0 / 3.0)))           # 436^3 = 82.9 M cells = 1440 x 1440 x 40
        vs = [(r[3] - r[0]) / side, (r[4] - r[1]) / side, (r[5] - r[2]) / side]
        p = torch.from_numpy(pts)
        mv, mp = cfg["max_voxels"][1], cfg["max_num_points"]

        def reference_cubic():
            vox = torch.zeros(mv, mp, pts.shape[1])
            coors = torch.zeros(mv, 3, dtype=torch.int32)
            npv = torch.zeros(mv, dtype=torch.int32)
            vext.hard_voxelize(p, vox, coors, npv, vs, list(r), mp, mv, 3, True)

        t_vox_ref, _ = _median_time(reference_cubic, runs=5, warmup=1)
    except Exception:
        pass
    coords4 = np.concatenate([np.zeros((c.shape[0], 1), np.int32), c], 1)
    enc = cpu_sparse_encoder_reference(coords4, cfg)
    spread = (max(bev_runs) - min(bev_runs)) / t_bev
    parts = [f"bev_pool: QuickCumsum pipeline (torch CPU, {threads} threads bound to cores = the fastest of a sweep over "
             f"{[e['threads'] for e in sweep]} threads on one camera's rows) on all {n_cam} cameras, N={ck.shape[0]} kept rows x {fk.shape[1]}, "
             f"median of 5 after 2 warm-ups = {t_bev * 1e3:.0f} ms, spread {spread:.2f} ({bev_bytes / t_bev / 1e9:.2f} GB/s on the "
             f"{bev_bytes / 1e6:.1f} MB of the scatter)",
             f"hard voxelize + mean of {pts.shape[0]} points: serial C restatement on 1440x1440x40, median of 5 = {t_vox * 1e3:.1f} ms "
             f"({pts.shape[0] / t_vox / 1e6:.1f} M points/s)"
             + (f"; reference hard_voxelize_cpu (oracle/_ref) on a 436^3 grid of equal cell count, median of 5 = {t_vox_ref * 1e3:.1f} ms"
                if t_vox_ref is not None else "; reference hard_voxelize_cpu not available on this box")]
    if enc is not None:
        parts.append(f"SparseEncoder via the reference's CPU functors (oracle/_ref, fp32, {physical} threads): one rulebook per geometry "
                     f"= {enc['seconds_once']:.2f} s, with the reference's recompute pattern (16 of 17 SubM rulebooks rebuilt; the measured "
                     f"per-level build times re-added) = {enc['seconds_recompute']:.2f} s")
        total, kind = t_bev + t_vox + enc["seconds_once"], "reference"
    else:
        parts.append("SparseEncoder: reference CPU build not available, stage omitted")
        total, kind = t_bev + t_vox, "port"
    out = dict(value=1.0 / total, unit="frames/s", cores=physical, kind=kind,
               sample_short=f"ONE frame, stage by stage, child process bound to cores: QuickCumsum bev_pool (torch CPU, {threads} thr) "
                            f"+ hard voxelize (serial C) + SparseEncoder (reference CPU functors, {physical} thr)",
               sample="one frame, stage by stage (BASELINE.md §3 protocol), in a child process with OMP_PLACES=cores OMP_PROC_BIND=close: "
                      + "; ".join(parts), seconds_per_frame=total,
               bev_pool_quickcumsum_ms=t_bev * 1e3, bev_pool_quickcumsum_runs_ms=[t * 1e3 for t in bev_runs],
               bev_pool_quickcumsum_spread=spread, bev_pool_quickcumsum_threads=threads,
               bev_pool_quickcumsum_thread_sweep_one_camera=sweep,
               threads_note=f"threads bound to physical cores (OMP_PLACES=cores, OMP_PROC_BIND=close) in a child process; QuickCumsum at the "
                            f"fastest thread count of the sweep ({threads}), the other stages at {physical}",
               bev_pool_gbs=bev_bytes / t_bev / 1e9, voxelize_restated_ms=t_vox * 1e3,
               voxelize_reference_cubic_ms=None if t_vox_ref is None else t_vox_ref * 1e3)
    if enc is not None:
        out.update(encoder_one_rulebook_per_stage_s=enc["seconds_once"], encoder_reference_recompute_s=enc["seconds_recompute"],
                   frames_per_s_reference_recompute=1.0 / (t_bev + t_vox + enc["seconds_recompute"]))
    print(json.dumps(out), flush=True)


def train_step(args, rank, world, frame_ids, dev):
    """`--mode train-step`: one optimisation step of the hot path's trainable part per timed step — BASELINE configs[4].
    camera: bev_pool forward + backward on the materialised [N', 80] volume (the API-level op; backward = 622.5 MB per frame,
    SURVEY.md §8d) and the fused depth (x) context pooling forward + backward (what DepthLSSTransform runs);
    LiDAR: hard voxelization (no gradient) + SparseEncoder forward / backward in fp32 training mode (module path, autograd:
    dgrad through the forward kernel on the transposed table, MFMA filter gradient), gradient all-reduce by
    DistributedDataParallel over RCCL when world > 1, clip_grad_norm 35 + AdamW(lr 2e-4) step (configs/default.yaml)."""
    import torch.distributed as dist

    from bevfusion_amd import synth
    from bevfusion_amd.bev_pool import BevPoolPlan
    from bevfusion_amd.sharding import barrier, max_over_ranks, sum_over_ranks
    from bevfusion_amd.voxel import voxelize_batch

    cfg = synth.CL_CONFIG
    B = len(frame_ids)
    augmented = getattr(args, "train_inputs", "augmented") == "augmented"
    inp = synth.bev_pool_inputs(cfg, batch=1, seed=rank, with_feats=False)     # one calibration, tiled over the frames on the device
    H, W, D = (int(v) for v in inp["nx"])
    C = inp["channels"]
    geom = torch.from_numpy(inp["geom"]).to(dev).repeat(B, 1)
    plan0 = BevPoolPlan.from_geometry(geom, B, inp["origin"], inp["dx"], inp["nx"], want_intervals=True)
    gen = torch.Generator(device=dev).manual_seed(99 + rank)
    feats = torch.randn((geom.shape[0], C), generator=gen, device=dev).requires_grad_(True)
    fh, fw = cfg["feature_size"]
    n_cam = cfg["num_cameras"]
    dbins = geom.shape[0] // (B * n_cam * fh * fw)
    depth = torch.softmax(torch.randn((B * n_cam, dbins, fh, fw), generator=gen, device=dev), 1).requires_grad_(True)
    ctx = torch.randn((B * n_cam * fh * fw, C), generator=gen, device=dev).requires_grad_(True)
    gout = torch.randn((B, D, H, W, C), generator=gen, device=dev)
    # ---- the inputs of a step.  augmented (VERDICT r5 missing #3): the reference augments per sample per step
    # (configs/nuscenes/default.yaml:13-15, 20-23; datasets/pipelines/transforms_3d.py:85-165, 196-230), so get_geometry
    # (vtransforms/base.py:92-135), the rank / sort / CSR plan (base.py:141-176, bev_pool.py:83-97) and the column plan of the fused
    # pooling are on the critical path of EVERY training step: they are rebuilt inside the timed step from that step's matrices
    # (drawn beforehand: sampling is the data loader's work), and the point clouds rotate through a pool with that step's LiDAR
    # augmentation applied.
    from bevfusion_amd.vtransforms import DepthLSSTransform

    vt = DepthLSSTransform(256, C, cfg["image_size"], cfg["feature_size"], cfg["xbound"], cfg["ybound"], cfg["zbound"], cfg["dbound"],
                           downsample=2).to(dev).eval()
    rig = synth.camera_rig(n_cam)
    t_c2l_r = torch.from_numpy(np.tile(rig["camera2lidar_rots"], (B, 1, 1, 1))).to(dev)
    t_c2l_t = torch.from_numpy(np.tile(rig["camera2lidar_trans"], (B, 1, 1))).to(dev)
    t_K = torch.from_numpy(np.tile(rig["intrins"], (B, 1, 1, 1))).to(dev)
    n_pool = max(8, 2 * B) if augmented else B
    pool = [torch.from_numpy(synth.lidar_points(seed=1000 * rank + f)).to(dev) for f in (range(n_pool) if augmented else frame_ids)]
    rng = np.random.default_rng(4242 + rank)
    n_aug = (max(1, args.warmup) + args.steps) if augmented else 0
    augs = []
    for _ in range(n_aug):
        a = synth.training_augmentation(rng, B, n_cam, cfg)
        augs.append({k: torch.from_numpy(v).to(dev) for k, v in a.items()})
    origin, dx_l, nx_l = inp["origin"], inp["dx"], inp["nx"]
    state = {"i": 0, "plan": plan0, "runs": [], "kernel": [], "kept": []}
    enc = make_encoder(cfg, dev, torch.float32).train()
    model = wrap_for_gradient_allreduce(enc, world, dev)
    opt = torch.optim.AdamW(enc.parameters(), lr=2e-4, weight_decay=0.01)
    scaler = torch.amp.GradScaler("cuda", growth_interval=2000) if args.amp else None
    # rows in key order (the voxelizer's default here) are in ascending linear index: the encoder trains on the inference kernels
    # (spconv/fused_train.py; --voxel-order first or BEVAMD_SPCONV_FUSED_TRAIN=0: the module-by-module path)
    coors_order = "linear" if args.voxel_order == "key" else None
    names = ["geometry+plan", "bev_pool_fwd", "bev_pool_bwd", "fused_pool_fwd", "fused_pool_bwd", "voxelize", "encoder_fwd", "encoder_bwd+allreduce",
             "clip+adamw"]
    last_step = max(1, args.warmup) + args.steps - 1          # index of the last timed step: its results are kept for --dump-outputs

    def step(ev=None):
        mark = (lambda i: ev[i].record()) if ev else (lambda i: None)
        i = state["i"]
        state["i"] += 1
        mark(0)
        if augmented:
            a = augs[i % n_aug]
            with torch.no_grad():
                gm = vt.get_geometry(t_c2l_r, t_c2l_t, t_K, a["post_rots"], a["post_trans"], extra_rots=a["extra_rots"],
                                     extra_trans=a["extra_trans"])
            plan = BevPoolPlan.from_geometry(gm.view(-1, 3), B, origin, dx_l, nx_l)
            plan.prepare_fused(dbins, fh, fw, C)             # the column plan (one 4-byte read-back sizes its buffers)
            state["plan"] = plan
            pts = []
            for j in range(B):
                p = pool[(i * B + j) % n_pool]
                xyz = p[:, :3] @ a["extra_rots"][j].t() + a["extra_trans"][j]       # the step's LiDAR augmentation on the device
                pts.append(torch.cat((xyz, p[:, 3:]), 1))
        else:
            plan, pts = plan0, pool
        mark(1)
        out = plan.forward(feats)
        mark(2)
        out.backward(gout)
        mark(3)
        outf = plan.fused(depth, ctx, dbins, fh, fw)
        mark(4)
        outf.backward(gout)
        mark(5)
        vf, vc, _ = voxelize_batch(pts, cfg["voxel_size"], cfg["point_cloud_range"], cfg["max_num_points"], cfg["max_voxels"][0],
                                   order=args.voxel_order)
        mark(6)
        if scaler is not None:
            with torch.autocast("cuda", dtype=torch.float16):
                y = model(vf, vc, B, coors_order=coors_order)
            mark(7)
            scaler.scale(y.float().square().mean()).backward()
            mark(8)
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(enc.parameters(), 35.0)
            scaler.step(opt)
            scaler.update()
        else:
            y = model(vf, vc, B, coors_order=coors_order)
            mark(7)
            y.square().mean().backward()
            mark(8)
            torch.nn.utils.clip_grad_norm_(enc.parameters(), 35.0)
            opt.step()
        opt.zero_grad(set_to_none=True)
        if args.dump_outputs and i == last_step:      # references only: no device work added to the step
            state["outputs"] = dict(bev_pool=out, fused_pool=outf, encoder_out=y, feats_grad=feats.grad, depth_grad=depth.grad,
                                    ctx_grad=ctx.grad)
        feats.grad = depth.grad = ctx.grad = None
        mark(9)
        if augmented and ev is None:        # warm-up steps only (untimed): which fused kernel the step's plan selects, runs per image column
            cols = plan.fused_columns(dbins, fh, fw, C, build=False)
            state["kernel"].append("columns" if cols is not None else "cells")
            if cols is not None:
                state["runs"].append(cols.nruns / max(1, B * n_cam * dbins * fw))

    for _ in range(max(1, args.warmup)):
        step()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)] for _ in range(args.steps)]
    barrier()
    torch.cuda.synchronize()
    with quiet_gc():
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(evs[i])
        torch.cuda.synchronize()
        barrier()
        elapsed_local = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        params = torch.cat([p.detach().reshape(-1).float() for p in enc.parameters()])      # the weights the step updated
        dump_outputs(args.dump_outputs, dict(state.pop("outputs"), encoder_params=params))
    elapsed = max_over_ranks(elapsed_local, device=dev)
    frames_per_step = int(sum_over_ranks(B, device=dev))
    stage = {n: float(np.mean([e[i].elapsed_time(e[i + 1]) for e in evs])) for i, n in enumerate(names)}
    per_step_ms = [round(float(e[0].elapsed_time(e[len(names)])), 3) for e in evs]            # GPU time of every timed step
    fwd_step_ms = [round(float(e[6].elapsed_time(e[7])), 3) for e in evs]                     # ... and of its encoder forward
    plan = state["plan"]
    n_kept = plan.n_kept()
    # the dominant streaming kernel of the step, timed on its own (the stage above also holds autograd's copy of the incoming gradient)
    for _ in range(3):
        plan.launch_backward(gout, C)
    kev = [torch.cuda.Event(enable_timing=True) for _ in range(21)]      # one event pair around EACH launch: the kernel's duration, as
    kev[0].record()                                                        # a kernel trace measures it (not the back-to-back rate)
    for i in range(20):
        plan.launch_backward(gout, C)
        kev[i + 1].record()
    kev[20].synchronize()
    bwd_kernel_ms = sum(kev[i].elapsed_time(kev[i + 1]) for i in range(20)) / 20
    res = None
    if rank == 0:
        bwd_bytes = B * D * H * W * C * 4 + n_kept * C * 4          # cell gradients read + row gradients written
        achieved = bwd_bytes / (bwd_kernel_ms * 1e-3) / 1e9
        nparam = sum(p.numel() for p in enc.parameters())
        res = ({
            "metric": "train-step frames/sec of the BEVFusion C+L hot path (fwd + bwd + optimizer step of bev_pool / fused pooling / "
                      "voxelize / SparseEncoder), " + ("fp16 mixed precision (the reference's default: configs/default.yaml fp16)" if args.amp else "fp32"),
            "value": frames_per_step * args.steps / elapsed, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong" if args.global_batch else "weak", "vs_baseline": None,
            "dtype": "f16 convolution operands / f32 accumulate, master weights, BatchNorm and pooling (autocast)" if args.amp else "f32",
            "data": "synthetic",
            "config": {"workload": f"training step of the hot path, {B} frame(s)/GPU (BASELINE configs[4]: 4 per GPU): bev_pool "
                                   f"N'={geom.shape[0]} ({n_kept} kept) x C={C} fwd+bwd, fused depth x context pooling fwd+bwd, hard "
                                   f"voxelize ~{sum(p.shape[0] for p in pool[:B])} points (cap {cfg['max_voxels'][0]}), SparseEncoder fp32 "
                                   f"train mode ({nparam} parameters) fwd+bwd, clip_grad_norm 35, AdamW",
                       "inputs": ("augmented per step like the reference's training pipeline: per-camera image augmentation (resize 0.38-0.55, "
                                  "rotate +-5.4 deg, flip), per-sample LiDAR augmentation (rotate +-45 deg, scale 0.9-1.1, translate N(0, 0.5 m)); "
                                  "get_geometry + pooling plan + column plan rebuilt INSIDE every timed step (stage geometry+plan); point clouds "
                                  f"rotate through a pool of {n_pool}") if augmented else
                                 "static (round 5 protocol): one test-time calibration, plan built once outside the timed loop, the same clouds every step",
                       "encoder_path": f"{enc.last_path}" + (f" ({enc.last_path_reason})" if enc.last_path_reason else ""),
                       "plan_ms": stage.get("geometry+plan"),
                       "runs_per_column": (float(np.mean(state["runs"])) if state["runs"] else None),
                       "fused_kernel": (max(set(state["kernel"]), key=state["kernel"].count) if state["kernel"] else "columns (static plan)"),
                       "frames_per_step_per_gpu": B, "frames_per_step": frames_per_step, "stage_ms": stage,
                       "per_step_ms": per_step_ms, "encoder_fwd_per_step_ms": fwd_step_ms,
                       "host_gc": "Python's cyclic collector is off inside the timed region (timeit's convention; see quiet_gc)",
                       "gradient_allreduce": (f"DistributedDataParallel over torch.distributed {_backend_name()}, world {world}, "
                                              f"{nparam * 4 / 1e6:.1f} MB per step") if world > 1 else "single rank: none"},
            "roofline": {"kernel": "bev_pool_bwd_points_vec_kernel", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                         "algorithmic_bytes_per_launch": bwd_bytes, "kernel_ms": bwd_kernel_ms,
                         "note": "average duration of 20 launches of the backward kernel, one HIP event pair around each (x_grad written in point order: a "
                                 "streaming write; the cell gradients it gathers stay in L2 / Infinity Cache); the bev_pool_bwd stage "
                                 "of the step also holds autograd's contiguous fp32 copy of the incoming gradient"},
            "cpu_baseline": None})
    return res


def main():
    args = parse()
    if args.cpu_baseline_worker:
        return cpu_baseline_worker(args.cpu_baseline_worker)
    if args.batch is None:
        args.batch = 4 if args.mode == "train-step" else 8
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(respawn_under_launcher(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and rank == 0:
        print(f"[bench] --gpus {args.gpus} but the launcher started {world} rank(s): using {world}", file=sys.stderr)
    if not args.dry_run and not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the HIP path has no CPU fallback); --dry-run exercises the launch logic")
    # tests on a ONE-GPU box (tests/test_gpu_bench_multirank.py): every rank on device 0, collectives over gloo — the whole N > 1
    # control flow of the REAL step (per-rank frames, plans, HIP graphs, barriers, max over ranks, rank-0 line) without a second GPU.
    # RCCL refuses two ranks on one device; the RCCL path itself is tests/test_gpu_ddp.py
    shared_gpu = os.environ.get("BEVAMD_BENCH_SHARED_GPU", "0") == "1"
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dry_run or shared_gpu:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))   # "nccl" == RCCL on ROCm

    from bevfusion_amd.sharding import frames_for_rank

    # frames of one step: weak scaling = --batch frames on every rank; strong = --global-batch split over the ranks
    if args.global_batch:
        frame_ids = list(frames_for_rank(args.global_batch, rank, world))
    else:
        frame_ids = [rank * max(1, args.batch) + b for b in range(max(1, args.batch))]
    if args.dry_run:
        from bevfusion_amd.sharding import bind_rank_to_cpus

        args.cpu_binding = bind_rank_to_cpus(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
        (dry_run_train if args.mode == "train-step" else dry_run)(args, rank, world, frame_ids)
        if world > 1:
            import torch.distributed as dist

            dist.destroy_process_group()
        return
    if not frame_ids:
        raise SystemExit(f"rank {rank}: no frames to process (--global-batch {args.global_batch} < {world} ranks)")
    dev = torch.device("cuda", 0 if shared_gpu else local_rank)
    torch.cuda.set_device(dev)
    from bevfusion_amd.sharding import bind_rank_to_cpus

    # one process per GPU on one host: each rank keeps to its share of the cores, next to its GPU (input synthesis, launches, timing)
    cpu_binding = bind_rank_to_cpus(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    args.cpu_binding = cpu_binding
    if args.mode == "train-step":
        res = train_step(args, rank, world, frame_ids, dev)
        if rank == 0:
            emit(res)
        if world > 1:
            import torch.distributed as dist

            dist.destroy_process_group()
        return

    from bevfusion_amd import synth
    from bevfusion_amd.bev_pool import BevPoolPlan
    from bevfusion_amd.voxel import voxelize_batch_device

    cfg = synth.CL_CONFIG
    B = len(frame_ids)
    # ---- synthetic frame (per rank: its own seed -> its own features / point cloud; same calibration) ----
    # every frame of a step shares the calibration: the frustum geometry is synthesised for ONE frame on the host (0.2 s; 2 s for
    # 8 — per rank, on its own cores) and tiled on the device
    inp = synth.bev_pool_inputs(cfg, batch=1, seed=rank, with_feats=False)
    H, W, D = (int(v) for v in inp["nx"])
    C = inp["channels"]
    geom = torch.from_numpy(inp["geom"]).to(dev).repeat(B, 1)
    # independent random features per frame and rank, drawn on the device (5 GB at 8 frames: minutes of host RNG + PCIe)
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    feats = torch.randn((geom.shape[0], C), generator=gen, device=dev, dtype=torch.float32)
    n_cam = cfg["num_cameras"]
    cpu_base = args.full and rank == 0 and world == 1 and not args.no_cpu_baseline
    inp["feats"] = feats[: geom.shape[0] // B].cpu().numpy() if cpu_base else None   # frame 0: the CPU baseline's sample
    if args.feat_dtype == "bf16":
        feats = feats.bfloat16()
    elem = feats.element_size()
    pts_all = [synth.lidar_points(seed=f) for f in frame_ids]                  # one point cloud per frame id
    pts_np = pts_all[0]
    pts_list = [torch.from_numpy(p).to(dev) for p in pts_all]
    sp_dtype = {"fp16": torch.float16, "fp32": torch.float32, "bf16": torch.bfloat16}[args.spconv_dtype]
    enc = make_encoder(cfg, dev, sp_dtype)

    # bev_pool precompute (cached per calibration at inference; timed separately, not inside the step)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = BevPoolPlan.from_geometry(geom, B, inp["origin"], inp["dx"], inp["nx"], want_intervals=True)
    torch.cuda.synchronize()
    t_first = time.perf_counter() - t0
    precompute_ms = None
    if args.full:
        t0 = time.perf_counter()
        for _ in range(5):
            plan = BevPoolPlan.from_geometry(geom, B, inp["origin"], inp["dx"], inp["nx"], want_intervals=True)
        torch.cuda.synchronize()
        precompute_ms = (time.perf_counter() - t0) / 5 * 1e3
    n_kept, n_int = plan.n_kept(), plan.n_intervals()
    bev = torch.empty((B, D, H, W, C), dtype=torch.float32, device=dev)

    state = {}
    coors_order = "linear" if args.voxel_order == "key" else None
    # the voxelizer's mean kernel writes the encoder's 16-bit input rows itself (no pad-and-cast pass in front of the first layer)
    enc_rows = sp_dtype if sp_dtype != torch.float32 else None

    def lidar_branch():
        # voxelize + mean into capacity-sized buffers, voxel count stays on the device (no host sync), then the
        # sparse encoder on its sync-free fused inference path
        vf, vc, _, cnt = voxelize_batch_device(pts_list, cfg["voxel_size"], cfg["point_cloud_range"], cfg["max_num_points"],
                                               cfg["max_voxels"][1], order=args.voxel_order, encoder_rows=enc_rows)
        mid = torch.cuda.Event(enable_timing=True) if state.get("probe") else None
        if mid is not None:
            mid.record()
        with torch.no_grad():
            out = enc(vf, vc, B, num_voxels=cnt, coors_order=coors_order)
        return out, cnt, mid

    from bevfusion_amd.sharding import barrier, max_over_ranks, sum_over_ranks

    # eager passes: warm every cache (filter images, allocator) and time voxelize / encoder separately
    for _ in range(2):
        lidar_branch()
    torch.cuda.synchronize()
    if sp_dtype != torch.float32 and enc.last_path != "fused":
        raise SystemExit(f"bench: the SparseEncoder left its sync-free fused path ({enc.last_path_reason})")
    eager_vox_ms = eager_enc_ms = None
    if args.full:
        state["probe"] = True
        sub = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _, _, mid = lidar_branch()
            b.record()
            b.synchronize()
            sub.append((a.elapsed_time(mid), mid.elapsed_time(b)))
        state["probe"] = False
        eager_vox_ms, eager_enc_ms = (float(np.median([t[i] for t in sub])) for i in (0, 1))

    # per-layer convolution figures (`roofline_spconv`): one eager pass with HIP events around every layer
    from bevfusion_amd.spconv import fused as _fused

    roofline_spconv = None
    if args.full and sp_dtype != torch.float32:
        _fused.LAYER_PROFILE = []
        _fused.LAYER_PROFILE_REPS = 5    # 5 back-to-back launches per layer between the events (a single launch behind a sync runs down-clocked)
        try:
            lidar_branch()
            layers = _fused.summarize_layer_profile(_fused.LAYER_PROFILE, elem_bytes=2)
        finally:
            _fused.LAYER_PROFILE = None
            _fused.LAYER_PROFILE_REPS = 1
        tot_us, tot_gf = sum(l["us"] for l in layers), sum(l["gflop"] for l in layers)
        # what the kernels ISSUE (every tap of an output-stationary tile, real pair or not) and the yardstick for it: the vendor
        # library's square fp16 GEMM on random operands on THIS box (matrix-dense bodies clock ~1.9 GHz: EXPERIMENTS D.9)
        dense_gf = sum(l["gflop"] / l["useful_mfma_fraction"] for l in layers if l.get("useful_mfma_fraction"))
        ga, gb = (torch.randn(4096, 4096, device=dev, dtype=torch.float16) for _ in range(2))
        for _ in range(3):
            torch.matmul(ga, gb)
        g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g0.record()
        for _ in range(20):
            torch.matmul(ga, gb)
        g1.record()
        g1.synchronize()
        gemm_tflops = 2.0 * 4096 ** 3 * 20 / (g0.elapsed_time(g1) * 1e-3) / 1e12
        del ga, gb
        roofline_spconv = {
            "note": "21 convolutions of the SparseEncoder, one eager pass with the rulebooks already built (HIP events around 5 back-to-back "
                    "launches of every layer, nothing beside them). FLOP = 2*pairs*Cin*Cout (real pairs only); ideal bytes = "
                    "N_in*Cin*2 + pairs*8 + K*Cin*Cout*2 + N_out*Cout*2 (SURVEY.md 8d). Peaks: 2.5 PFLOP/s dense fp16 MFMA, 8 TB/s. "
                    "The op is neither: rows live in L2 and 133 GFLOP/frame is < 0.1 ms of MFMA — fractions are for orientation.",
            "total_us": tot_us, "total_gflop": tot_gf, "tflops": tot_gf * 1e3 / tot_us, "frac_mfma_peak": tot_gf * 1e3 / tot_us / 2500.0,
            "n_layers": len(layers),
            "dense_tap_tflops": dense_gf * 1e3 / tot_us, "gemm_yardstick_tflops": gemm_tflops,
            "dense_tap_frac_of_gemm_yardstick": dense_gf * 1e3 / tot_us / gemm_tflops,
            "yardstick": "torch.matmul (hipBLASLt) 4096^3 fp16 on random operands, 20 launches between HIP events, measured in this run",
            "layers": [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in l.items()} for l in layers],
        }

    if args.overlap == "auto":
        args.overlap = ("ahead" if B >= 2 else "voxel") if (sp_dtype != torch.float32 and not args.no_graph) else "none"
    overlap_head = args.overlap == "head" and sp_dtype != torch.float32 and not args.no_graph
    overlap_voxel = args.overlap == "voxel" and sp_dtype != torch.float32 and not args.no_graph
    overlap_pipe = args.overlap == "pipeline" and sp_dtype != torch.float32 and not args.no_graph
    overlap_chain = args.overlap == "chain" and sp_dtype != torch.float32 and not args.no_graph
    # ahead: software pipeline ACROSS steps — the coordinate-only half of the LiDAR branch (voxelizer + the encoder's whole rulebook
    # chain: latency-bound integer kernels) of batch t + 1 runs underneath the convolutions of batch t; two buffer sets alternate
    overlap_ahead = args.overlap == "ahead" and sp_dtype != torch.float32 and not args.no_graph
    ahead_gate = os.environ.get("BEVAMD_BENCH_AHEAD_GATE", "step")   # when the next batch's head may start: step | fused | bev_pool
    # ahead, BEVAMD_BENCH_BEVPOOL_ALONE=1: the API-level bev_pool kernel first and ALONE, every other stream of the step forked behind
    # it — the roofline kernel at its solo rate INSIDE the timed step (0.61-0.62 of 8 TB/s in the step against 0.36-0.37) for 2.5 % of
    # the step (4.53 against 4.42 ms, three interleaved pairs on one box); the default keeps the faster schedule and reports this one
    # as extra.alone_step_ms / alone_frac_in_step
    bev_pool_alone = overlap_ahead and os.environ.get("BEVAMD_BENCH_BEVPOOL_ALONE", "0") == "1"
    chain_gate = os.environ.get("BEVAMD_BENCH_CHAIN_GATE", "1") != "0"   # A/B: 0 lets the chain start as soon as the voxelizer is done

    def lidar_head():
        """coordinates only: voxelize + mean, then the encoder's whole rulebook chain (hash, active sets, neighbour tables, slab
        metadata of every level) — SparseEncoder.prepare_geometry"""
        vf, vc, _, cnt = voxelize_batch_device(pts_list, cfg["voxel_size"], cfg["point_cloud_range"], cfg["max_num_points"],
                                               cfg["max_voxels"][1], order=args.voxel_order, encoder_rows=enc_rows)
        with torch.no_grad():
            lvl = enc.prepare_geometry(vc, B, num_voxels=cnt, coors_order=coors_order)
        return vf, vc, cnt, lvl

    def lidar_tail(vf, vc, cnt, lvl):
        with torch.no_grad():
            if lvl is None:   # --overlap voxel: the encoder builds (and overlaps) its own rulebook chain
                return enc(vf, vc, B, num_voxels=cnt, coors_order=coors_order)
            return enc(vf, vc, B, num_voxels=cnt, geometry=lvl)

    def voxel_head(pl=None):
        vf, vc, _, cnt = voxelize_batch_device(pts_list if pl is None else pl, cfg["voxel_size"], cfg["point_cloud_range"], cfg["max_num_points"],
                                               cfg["max_voxels"][1], order=args.voxel_order, encoder_rows=enc_rows)
        return vf, vc, cnt, None

    if overlap_voxel:
        lidar_head = voxel_head
        overlap_head = True   # same fork / join around the camera stages, a shorter head

    def geometry_head(vf, vc, cnt, _):
        with torch.no_grad():
            return vf, vc, cnt, enc.prepare_geometry(vc, B, num_voxels=cnt, coors_order=coors_order)

    graph = graph_head = graph_tail = None
    overlap_lidar = args.overlap == "lidar" and not args.no_graph
    head_prio = int(os.environ.get("BEVAMD_BENCH_HEAD_PRIO", "0"))   # A/B: -1 = the second stream (LiDAR) as a high-priority HIP stream
    head_stream = torch.cuda.Stream(priority=head_prio) if (overlap_head or overlap_lidar or overlap_pipe or overlap_chain or overlap_ahead) else None
    graph_vox = graph_geo = None
    ahead_sets = None
    if not args.no_graph:
        # the LiDAR branch has no host sync: capture it once, replay it per frame (HIP graph, one launch)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            if overlap_head:
                lidar_tail(*lidar_head())
            elif overlap_pipe or overlap_chain or overlap_ahead:
                lidar_tail(*geometry_head(*voxel_head()))
            else:
                lidar_branch()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if overlap_pipe or overlap_chain:
            graph_vox = new_graph()
            with torch.cuda.graph(graph_vox):
                state["vox"] = voxel_head()
            graph_geo = new_graph()
            with torch.cuda.graph(graph_geo, pool=graph_vox.pool()):
                state["head"] = geometry_head(*state["vox"])
            graph_tail = new_graph()
            with torch.cuda.graph(graph_tail, pool=graph_vox.pool()):
                state["lidar_bev"] = lidar_tail(*state["head"])
            state["n_voxels_dev"] = state["head"][2]
            assert enc.last_path == "fused", enc.last_path_reason
        elif overlap_ahead:
            # two buffer sets, each with its own point clouds (set 1: other seeds), its own head graph (voxelizer + rulebook chain)
            # and its own tail graph (21 convolutions + dense tail) in ONE private pool per set: head and tail of a set never run at
            # the same time, the two sets do
            pts_b = [torch.from_numpy(synth.lidar_points(seed=100003 + f)).to(dev) for f in frame_ids]
            ahead_sets = []
            for pl in (pts_list, pts_b):
                with torch.cuda.stream(side):   # eager warm-up of this set's inputs
                    lidar_tail(*geometry_head(*voxel_head(pl)))
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                gh = new_graph()
                with torch.cuda.graph(gh):
                    hd = geometry_head(*voxel_head(pl))
                gt = new_graph()
                with torch.cuda.graph(gt, pool=gh.pool()):
                    out = lidar_tail(*hd)
                ahead_sets.append(dict(pts=pl, head=gh, tail=gt, hd=hd, out=out))
            state["lidar_bev"], state["n_voxels_dev"] = ahead_sets[0]["out"], ahead_sets[0]["hd"][2]
            assert enc.last_path == "fused", enc.last_path_reason
        elif overlap_head:
            graph_head = new_graph()
            with torch.cuda.graph(graph_head):
                state["head"] = lidar_head()
            graph_tail = new_graph()
            with torch.cuda.graph(graph_tail):
                state["lidar_bev"] = lidar_tail(*state["head"])
            state["n_voxels_dev"] = state["head"][2]
            assert enc.last_path == "fused", enc.last_path_reason
        else:
            graph = new_graph()
            with torch.cuda.graph(graph):
                state["lidar_bev"], state["n_voxels_dev"], _ = lidar_branch()

    # ---- camera branch as the product runs it: the step starts from what the dense network hands over ----
    # depth distribution [B*6, 118, 32, 88] (softmax output of depthnet), context [B*6*32*88, 80] (channels-last), the LiDAR
    # points and the calibration matrices:
    #   depth raster  (base.py:283-329, a3)  points -> [B, 6, 1, 256, 704] scalar depth images (input of dtransform, which is
    #                                        dense torch.nn and out of scope; its output stands in as the random `depth_prob`)
    #   fused pooling (depth_lss.py:92-97 + base.py:141-176, a4-a8)  out[cell] = sum depth * ctx, the [N', 80] volume never built
    # The geometry / pooling plan is static per calibration at inference (cached; its uncached cost is reported next to it).
    # The materialised-volume bev_pool kernel stays a stage of the step as well: it is the API-level op BASELINE.json's
    # "bev_pool HBM GB/s" is defined on — the camera reduction is therefore paid twice in `value`.
    from bevfusion_amd.vtransforms import DepthLSSTransform

    fh, fw = cfg["feature_size"]
    n_cam = cfg["num_cameras"]
    dbins = geom.shape[0] // (B * n_cam * fh * fw)
    vt = DepthLSSTransform(256, C, cfg["image_size"], cfg["feature_size"], cfg["xbound"], cfg["ybound"], cfg["zbound"],
                           cfg["dbound"], downsample=2).to(dev).eval()
    rig = synth.camera_rig(n_cam)
    mats = {}
    for name, (rot, trans) in dict(c2l=(rig["camera2lidar_rots"], rig["camera2lidar_trans"]),
                                   K=(rig["intrins"], np.zeros((n_cam, 3), np.float32)),
                                   ia=(rig["post_rots"], rig["post_trans"])).items():
        m4 = np.tile(np.eye(4, dtype=np.float32), (B, n_cam, 1, 1))
        m4[:, :, :3, :3], m4[:, :, :3, 3] = rot, trans
        mats[name] = m4
    l2i = (mats["K"].astype(np.float64) @ np.linalg.inv(mats["c2l"].astype(np.float64))).astype(np.float32)
    t_l2i, t_ia = torch.from_numpy(l2i).to(dev), torch.from_numpy(mats["ia"]).to(dev)
    t_la = torch.eye(4, device=dev).repeat(B, 1, 1)
    t_c2l, t_K = torch.from_numpy(mats["c2l"]).to(dev), torch.from_numpy(mats["K"]).to(dev)
    img_stub = torch.zeros(B, n_cam, 1, 1, 1, device=dev)
    g = torch.Generator(device=dev).manual_seed(7 + rank)
    depth_prob = torch.softmax(torch.randn((B * n_cam, dbins, fh, fw), generator=g, device=dev), 1)
    ctx_cl = torch.randn((B * n_cam * fh * fw, C), generator=g, device=dev)
    fused_out = torch.empty_like(bev)
    fused_bytes = n_kept * 4 + ctx_cl.numel() * 4 + B * D * H * W * C * 4

    def camera_geometry_uncached():
        """what a NEW calibration costs: device-side 3x3 inverses + frustum geometry + rank/sort/CSR plan (no host sync)"""
        with torch.no_grad():
            gm = vt.get_geometry(t_c2l[..., :3, :3], t_c2l[..., :3, 3], t_K[..., :3, :3], t_ia[..., :3, :3], t_ia[..., :3, 3],
                                 extra_rots=t_la[:, :3, :3], extra_trans=t_la[:, :3, 3])
            return vt.make_plan(gm, B)

    geometry_plan_ms = None
    if args.full:
        for _ in range(2):
            camera_geometry_uncached()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            camera_geometry_uncached()
        torch.cuda.synchronize()
        geometry_plan_ms = (time.perf_counter() - t0) / 5 * 1e3

    STAGES = ["depth_raster", "fused_depth_context_pool", "bev_pool_forward_cells",
              "voxelize_mean + sparse_encoder" if not overlap_head else
              ("join + sparse_encoder (the voxelizer ran beside the first camera stages on a second stream)" if overlap_voxel else
               "join + sparse_encoder convolutions (voxelize + rulebooks ran beside the camera stages on a second stream)")]
    if overlap_pipe:
        STAGES = ["bev_pool_forward_cells (voxelizer beside it on a second stream)",
                  "depth_raster (rulebook chain beside it)", "fused_depth_context_pool (rulebook chain beside it)",
                  "join + sparse_encoder convolutions"]
    if overlap_chain:
        STAGES = ["depth_raster (voxelizer beside it on a second stream)", "fused_depth_context_pool (voxelizer beside it)",
                  "bev_pool_forward_cells (the encoder's rulebook chain beside it)", "join + sparse_encoder convolutions + dense tail, alone"]
    if overlap_ahead:
        STAGES = ["depth_raster (this batch's convolutions beside it on a second stream)", "fused_depth_context_pool (convolutions beside it)",
                  "bev_pool_forward_cells (convolutions beside it)",
                  "join: rest of this batch's convolutions + dense tail, with the NEXT batch's voxelizer + rulebook chain beside them"]
    NSTAGE = len(STAGES)
    bp_done = torch.cuda.Event() if overlap_pipe else None
    fused_done = torch.cuda.Event() if overlap_chain else None

    def step_chain(ev=None, with_bev_pool=True):
        main_stream = torch.cuda.current_stream()
        head_stream.wait_stream(main_stream)                                  # fork
        with torch.cuda.stream(head_stream):
            graph_vox.replay()                                                # LiDAR: voxelizer, beside raster + fused pooling
        if ev:
            ev[0].record()
        with torch.no_grad():
            state["depth_img"] = vt.depth_raster(img_stub, pts_list, t_l2i, t_ia, t_la)
        if ev:
            ev[1].record()
        plan.launch_fused(depth_prob.view(-1), ctx_cl, dbins, fh, fw, out=fused_out)
        if chain_gate:
            fused_done.record(main_stream)
            head_stream.wait_event(fused_done)                                # the chain starts with bev_pool, not under the fused pooling
        with torch.cuda.stream(head_stream):
            graph_geo.replay()                                                # LiDAR: rulebook chain, beside bev_pool
        if ev:
            ev[2].record()
        if with_bev_pool:
            plan.launch_forward(feats, bev)                                   # the API-level bev_pool op (one kernel)
        if ev:
            ev[3].record()
        main_stream.wait_stream(head_stream)                                  # join
        graph_tail.replay()                                                   # LiDAR: the 21 convolutions + dense tail, alone
        if ev:
            ev[4].record()

    def step_pipeline(ev=None):
        main_stream = torch.cuda.current_stream()
        head_stream.wait_stream(main_stream)                                  # fork
        with torch.cuda.stream(head_stream):
            graph_vox.replay()                                                # LiDAR: voxelizer, beside bev_pool
        if ev:
            ev[0].record()
        plan.launch_forward(feats, bev)                                       # the API-level bev_pool op (one kernel; roofline)
        bp_done.record(main_stream)
        if ev:
            ev[1].record()
        with torch.cuda.stream(head_stream):
            head_stream.wait_event(bp_done)
            graph_geo.replay()                                                # LiDAR: rulebook chain, beside raster + fused pooling
        with torch.no_grad():
            state["depth_img"] = vt.depth_raster(img_stub, pts_list, t_l2i, t_ia, t_la)
        if ev:
            ev[2].record()
        plan.launch_fused(depth_prob.view(-1), ctx_cl, dbins, fh, fw, out=fused_out)
        if ev:
            ev[3].record()
        main_stream.wait_stream(head_stream)                                  # join
        graph_tail.replay()                                                   # LiDAR: the 21 convolutions + dense tail, alone
        if ev:
            ev[4].record()

    ahead_stream = torch.cuda.Stream() if overlap_ahead else None
    state["bev_pool_alone"] = bev_pool_alone
    ahead_ev = torch.cuda.Event() if overlap_ahead else None
    state["phase"] = 0

    def ahead_prime():
        """the head of the batch the next step convolves (untimed: warm-up does it once; every timed step pays for its successor's)"""
        ahead_sets[state["phase"]]["head"].replay()

    def step_ahead(ev=None, with_bev_pool=True, pl=None, alone=None):
        pl = pl or plan
        bev_pool_alone = state.get("bev_pool_alone", False) if alone is None else alone
        cur, nxt = ahead_sets[state["phase"]], ahead_sets[state["phase"] ^ 1]
        main_stream = torch.cuda.current_stream()
        if ev:
            ev[0].record()
        if bev_pool_alone:
            # the API-level bev_pool op (one kernel; roofline) FIRST and with nothing beside it: every other stream forks behind it.
            # Beside the convolutions the HBM stream and the layers slow each other by more than they overlap (EXPERIMENTS D.15)
            if with_bev_pool:
                pl.launch_forward(feats, bev)
            if ev:
                ev[1].record()
        head_stream.wait_stream(main_stream)                                  # fork
        ahead_stream.wait_stream(main_stream)
        with torch.cuda.stream(head_stream):
            cur["tail"].replay()                                              # LiDAR, batch t: 21 convolutions + dense tail (its head ran during step t - 1)
        if ahead_gate == "step" or bev_pool_alone:
            with torch.cuda.stream(ahead_stream):
                nxt["head"].replay()
        with torch.no_grad():
            state["depth_img"] = vt.depth_raster(img_stub, cur["pts"], t_l2i, t_ia, t_la)
        if ev:
            ev[2 if bev_pool_alone else 1].record()
        pl.launch_fused(depth_prob.view(-1), ctx_cl, dbins, fh, fw, out=fused_out)
        if ahead_gate == "fused" and not bev_pool_alone:
            ahead_ev.record(main_stream)
            with torch.cuda.stream(ahead_stream):
                ahead_stream.wait_event(ahead_ev)
                nxt["head"].replay()
        if ev:
            ev[3 if bev_pool_alone else 2].record()
        if not bev_pool_alone:
            if with_bev_pool:
                pl.launch_forward(feats, bev)                               # the API-level bev_pool op, beside the LiDAR streams
            if ahead_gate not in ("step", "fused"):
                ahead_ev.record(main_stream)
                with torch.cuda.stream(ahead_stream):
                    ahead_stream.wait_event(ahead_ev)                         # LiDAR, batch t + 1: voxelizer + rulebook chain, behind the HBM stream,
                    nxt["head"].replay()                                      # underneath the wide convolutions of batch t
            if ev:
                ev[3].record()
        main_stream.wait_stream(head_stream)                                  # join: batch t is complete
        main_stream.wait_stream(ahead_stream)                                 # ... and so is the head of batch t + 1
        state["lidar_bev"], state["n_voxels_dev"] = cur["out"], cur["hd"][2]
        state["phase"] ^= 1
        if ev:
            ev[4].record()

    # --overlap voxel: where the voxelizer's stream joins.  Several frames per step: in front of bev_pool — the voxelizer (0.3-0.5 ms
    # beside the camera kernels) outlasts the raster + fused pooling stages by a few tens of microseconds since the raster got faster,
    # and bev_pool's roofline figure is that of a kernel running alone (1.09 -> 1.03 ms; the wait shows in the fused pooling stage).
    # One or two frames: in front of the encoder — the voxelizer (0.12 ms) is LONGER than the two camera stages, and bev_pool is
    # the only thing left to hide it under (0.93-0.96 against 1.02-1.03 ms per single-frame step).
    early_join = overlap_voxel and B >= 4

    def step(ev=None):
        if overlap_pipe:
            return step_pipeline(ev)
        if overlap_chain:
            return step_chain(ev)
        if overlap_ahead:
            return step_ahead(ev)
        main_stream = torch.cuda.current_stream()
        if overlap_head:   # fork: LiDAR head on its own stream, underneath the camera stages
            head_stream.wait_stream(main_stream)
            with torch.cuda.stream(head_stream):
                graph_head.replay()
        if overlap_lidar:  # fork: the whole LiDAR branch beside the camera stages
            head_stream.wait_stream(main_stream)
            with torch.cuda.stream(head_stream):
                graph.replay()
        if ev:
            ev[0].record()
        with torch.no_grad():
            state["depth_img"] = vt.depth_raster(img_stub, pts_list, t_l2i, t_ia, t_la)   # camera: LiDAR -> depth images
        if ev:
            ev[1].record()
        plan.launch_fused(depth_prob.view(-1), ctx_cl, dbins, fh, fw, out=fused_out)      # camera: depth (x) context -> BEV
        if early_join:
            main_stream.wait_stream(head_stream)                          # join: the voxelizer has finished before bev_pool starts
        if ev:
            ev[2].record()
        plan.launch_forward(feats, bev)                                   # the API-level bev_pool op (one kernel; roofline)
        if ev:
            ev[3].record()
        if overlap_head:
            if not early_join:
                main_stream.wait_stream(head_stream)                      # join
            graph_tail.replay()                                           # LiDAR: the 21 convolutions + dense tail
        elif overlap_lidar:
            main_stream.wait_stream(head_stream)                          # join: what is left of the LiDAR branch
        elif graph is not None:
            graph.replay()                                                # LiDAR: voxelize + sparse encoder
        else:
            state["lidar_bev"], state["n_voxels_dev"], _ = lidar_branch()
        if ev:
            ev[4].record()

    if overlap_ahead:
        ahead_prime()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(NSTAGE + 1)] for _ in range(args.steps)]
    barrier()
    torch.cuda.synchronize()
    with quiet_gc():
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(evs[i])
        torch.cuda.synchronize()
        barrier()
        elapsed = time.perf_counter() - t0
    stage_ms = [float(np.mean([e[s].elapsed_time(e[s + 1]) for e in evs])) for s in range(NSTAGE)]
    state["n_voxels"] = int(state["n_voxels_dev"].reshape(-1)[0])
    assert tuple(state["lidar_bev"].shape) == (B, 256, 180, 180)
    if args.dump_outputs and rank == 0:   # before anything after the timed region launches into the same buffers
        dump_outputs(args.dump_outputs, dict(depth_raster=state["depth_img"], fused_pool=fused_out, bev_pool=bev,
                                             lidar_bev=state["lidar_bev"], n_voxels=state["n_voxels_dev"]))
    if overlap_pipe or bev_pool_alone:   # report in the canonical order (raster, fused pooling, bev_pool, LiDAR)
        stage_ms = [stage_ms[1], stage_ms[2], stage_ms[0], stage_ms[3]]
    kern_ms = stage_ms[2]  # the bev_pool stage is exactly one kernel launch
    fused_ms = stage_ms[1]

    box_sampled = box_info(dev.index or 0) if rank == 0 else None   # clocks right behind the timed region
    elapsed_local = elapsed
    elapsed = max_over_ranks(elapsed, device=dev)  # slowest rank defines the step time
    frames_per_step = int(sum_over_ranks(B, device=dev))
    rccl_ranks = int(sum_over_ranks(1, device=dev))  # world size as an all-reduce of ones over the backend sees it (RCCL when N > 1)

    # ---- secondary measurements, AFTER the timed region, one rank only: each is a driver-run figure of a
    # configuration the headline does not exercise.  Nothing here touches `value`.
    def timed(fn, n, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        with quiet_gc():
            t = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n * 1e3

    def kernel_ms(fn, n=20, warm=3):
        for _ in range(warm):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    extra = None
    def add_counts(a, b):
        return None if a is None or b is None else {k: a[k] + b[k] for k in a}

    # the roofline kernel SOLO (all ranks, right after the timed region): under --overlap chain the in-step launch shares the
    # machine with the rulebook chain; the roofline figure of the kernel itself is that of an undisturbed launch
    shared = overlap_chain or overlap_lidar or (overlap_head and not overlap_voxel) or overlap_pipe or overlap_ahead
    # Round 6 (the line's frac must follow from the committed kernel trace): the solo figure is the average DURATION
    # of a launch — one HIP event pair around EACH of 20 launches, which is what rocprofv3's kernel trace measures (an event between
    # two launches is a barrier: no overlap) — not the back-to-back rate of 20 launches, in which a launch's first workgroups start
    # while the previous launch drains (0.88 against 0.94 ms on one box: 0.71 against 0.66 of the peak).  The back-to-back rate
    # stays in the line as kernel_ms_back_to_back.
    def kernel_duration_ms(fn, n=20, warm=2):
        for _ in range(warm):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            fn()
            ev[i + 1].record()
        ev[n].synchronize()
        return sum(ev[i].elapsed_time(ev[i + 1]) for i in range(n)) / n

    solo_b2b_ms = kernel_ms(lambda: plan.launch_forward(feats, bev), n=20, warm=2) if shared and args.full else None
    solo_ms = kernel_duration_ms(lambda: plan.launch_forward(feats, bev)) if shared and args.full else None

    if args.full and rank == 0 and world == 1 and not args.no_extras and ((args.overlap == "none" and graph is not None) or overlap_voxel or overlap_chain or overlap_lidar or overlap_ahead):
        extra = {}
        t_extra = time.perf_counter()
        # (iv) the product's step: what a deployment runs per batch — raster + fused pooling + LiDAR branch — without the API-level
        # bev_pool kernel on the materialised volume (the camera reduction is otherwise counted twice in `value`); same schedule as
        # the headline step
        def product_step():
            if overlap_chain:
                return step_chain(None, with_bev_pool=False)
            if overlap_ahead:
                return step_ahead(None, with_bev_pool=False)
            main_stream = torch.cuda.current_stream()
            if overlap_lidar:
                head_stream.wait_stream(main_stream)
                with torch.cuda.stream(head_stream):
                    graph.replay()
            if overlap_voxel:
                head_stream.wait_stream(main_stream)
                with torch.cuda.stream(head_stream):
                    graph_head.replay()
            with torch.no_grad():
                state["depth_img"] = vt.depth_raster(img_stub, pts_list, t_l2i, t_ia, t_la)
            plan.launch_fused(depth_prob.view(-1), ctx_cl, dbins, fh, fw, out=fused_out)
            if overlap_voxel:
                main_stream.wait_stream(head_stream)
                graph_tail.replay()
            elif overlap_lidar:
                main_stream.wait_stream(head_stream)
            else:
                graph.replay()

        pm = timed(product_step, args.steps)
        extra["product_step"] = dict(ms_per_step=pm, frames_per_s=B * 1e3 / pm, frames=B,
                                     note="depth raster + fused depth x context pooling + LiDAR branch (schedule of the headline "
                                          "step); the API-level bev_pool kernel of the headline step left out")
        extra["lidar_graph"] = (add_counts(graph_node_count(ahead_sets[0]["head"]), graph_node_count(ahead_sets[0]["tail"])) if overlap_ahead else
                                add_counts(graph_node_count(graph_head), graph_node_count(graph_tail)) if overlap_voxel
                                else add_counts(add_counts(graph_node_count(graph_vox), graph_node_count(graph_geo)),
                                                graph_node_count(graph_tail)) if overlap_chain else graph_node_count(graph))
        if overlap_chain:
            def lidar_alone():
                graph_vox.replay()
                graph_geo.replay()
                graph_tail.replay()

            extra["lidar_branch_alone"] = dict(ms=kernel_ms(lidar_alone), frames=B,
                                               note="voxelizer, rulebook-chain and convolution graphs back to back on one stream, HIP events around 20 passes")
        if overlap_ahead:
            def lidar_alone():
                ahead_sets[0]["head"].replay()
                ahead_sets[0]["tail"].replay()

            def tail_alone():
                ahead_sets[0]["tail"].replay()

            extra["lidar_branch_alone"] = dict(ms=kernel_ms(lidar_alone), frames=B, convolutions_alone_ms=kernel_ms(tail_alone),
                                               note="head graph (voxelizer + rulebook chain) + tail graph (21 convolutions + dense tail) of one buffer "
                                                    "set back to back on one stream, HIP events around 20 passes; convolutions_alone_ms: the tail graph only")
            # the un-pipelined schedule of rounds 5-6 on the same box, same inputs: the whole LiDAR branch of THIS batch beside the camera stages
            def step_unpipelined():
                main_stream = torch.cuda.current_stream()
                head_stream.wait_stream(main_stream)
                with torch.cuda.stream(head_stream):
                    ahead_sets[0]["head"].replay()
                    ahead_sets[0]["tail"].replay()
                with torch.no_grad():
                    state["depth_img"] = vt.depth_raster(img_stub, pts_list, t_l2i, t_ia, t_la)
                plan.launch_fused(depth_prob.view(-1), ctx_cl, dbins, fh, fw, out=fused_out)
                plan.launch_forward(feats, bev)
                main_stream.wait_stream(head_stream)

            um = timed(step_unpipelined, args.steps)
            extra["unpipelined_step"] = dict(ms_per_step=um, frames_per_s=B * 1e3 / um, frames=B,
                                             note="every batch's voxelizer + rulebook chain + convolutions inside its own step (one stream beside the "
                                                  "camera stages: the `lidar` schedule with the chain in front of the convolutions instead of four layers ahead)")
            ahead_prime()   # restore the pipeline's invariant for whatever replays a step after this
            # the pipelined step computes what the plain encoder computes: batch 0's output against an eager pass over the same clouds
            with torch.no_grad():
                vf0, vc0, _, cnt0 = voxelize_batch_device(pts_list, cfg["voxel_size"], cfg["point_cloud_range"], cfg["max_num_points"],
                                                          cfg["max_voxels"][1], order=args.voxel_order, encoder_rows=enc_rows)
                ref0 = enc(vf0, vc0, B, num_voxels=cnt0, coors_order=coors_order)
            state["phase"] = 0
            step_ahead()
            torch.cuda.synchronize()
            extra["ahead_output_equals_eager"] = bool(torch.equal(ahead_sets[0]["out"], ref0))
            del ref0, vf0, vc0
        if overlap_voxel:
            # the LiDAR branch with nothing beside it (what stage_ms.lidar_branch measured up to round 3: under the default
            # schedule that stage no longer contains the voxelizer, which runs beside the raster / fused pooling stages)
            def lidar_alone():
                graph_head.replay()
                graph_tail.replay()

            extra["lidar_branch_alone"] = dict(ms=kernel_ms(lidar_alone), frames=B,
                                               note="voxelizer graph + encoder graph back to back on one stream, HIP events around 20 passes")
        # (v) the fused pooling alone, on the benchmark's rig (no pitch / roll: one run per image column, the best case of the
        # column formulation) and on a pitched / rolled rig (VERDICT r4 missing #5, weak #7): same sizes, its own plan
        try:
            fp = dict(alone_ms=kernel_ms(lambda: plan.launch_fused(depth_prob.view(-1), ctx_cl, dbins, fh, fw, out=fused_out)), frames=B)
            rg = synth.rigged_geometry(1, n_cam, dbins, fh, fw, seed=5, pitch_deg=1.5, roll_deg=1.0, rot_deg=0.0, flip=False)
            plan_r = BevPoolPlan.from_geometry(torch.from_numpy(rg.reshape(-1, 3)).to(dev).repeat(B, 1), B, inp["origin"], inp["dx"], inp["nx"])
            plan_r.prepare_fused(dbins, fh, fw, C)
            cols_r = plan_r.fused_columns(dbins, fh, fw, C)
            fp["rigged_ms"] = kernel_ms(lambda: plan_r.launch_fused(depth_prob.view(-1), ctx_cl, dbins, fh, fw, out=fused_out))
            fp["rigged_runs_per_column"] = None if cols_r is None else cols_r.nruns / max(1, B * n_cam * dbins * fw)
            cols_0 = plan.fused_columns(dbins, fh, fw, C)
            fp["runs_per_column"] = None if cols_0 is None else cols_0.nruns / max(1, B * n_cam * dbins * fw)
            fp["note"] = ("HIP events around 20 launches, nothing beside them; rigged: every camera pitched within +-1.5 deg and rolled "
                          "within +-1 deg (synth.rigged_geometry, seed 5), no image rotation / flip")
            extra["fused_pool"] = fp
            del plan_r
            if overlap_ahead:
                # (v') VERDICT r5 weak #7 / #11: the WHOLE step on a rig that is not the easy case — every frame its own calibration,
                # cameras pitched +-1.5 deg and rolled +-1 deg, no image rotation / flip (test time) — same sizes, its own plans
                rgv = synth.rigged_geometry(B, n_cam, dbins, fh, fw, seed=11 + rank, pitch_deg=1.5, roll_deg=1.0, rot_deg=0.0, flip=False)
                plan_v = BevPoolPlan.from_geometry(torch.from_numpy(rgv.reshape(-1, 3)).to(dev), B, inp["origin"], inp["dx"], inp["nx"])
                plan_v.prepare_fused(dbins, fh, fw, C)
                cols_v = plan_v.fused_columns(dbins, fh, fw, C)
                vm = timed(lambda: step_ahead(None, pl=plan_v), args.steps)
                extra["varied_rig_step"] = dict(ms_per_step=vm, frames_per_s=B * 1e3 / vm, frames=B, n_kept=plan_v.n_kept(),
                                                runs_per_column=None if cols_v is None else cols_v.nruns / max(1, B * n_cam * dbins * fw),
                                                note="the headline step with a different calibration per frame: every camera of every frame "
                                                     "pitched within +-1.5 deg and rolled within +-1 deg (synth.rigged_geometry), plans built "
                                                     "outside the step as at inference")
                del plan_v
                # (v'') the step with the API-level bev_pool kernel FIRST and ALONE (every other stream forked behind it): what the
                # roofline kernel does INSIDE a step when nothing shares the machine with it, and what that schedule costs
                am = timed(lambda: step_ahead(None, alone=True), args.steps)
                aevs = [[torch.cuda.Event(enable_timing=True) for _ in range(NSTAGE + 1)] for _ in range(10)]
                for e5 in aevs:
                    step_ahead(e5, alone=True)
                torch.cuda.synchronize()
                ak = float(np.mean([e5[0].elapsed_time(e5[1]) for e5 in aevs]))
                extra["bev_pool_alone_step"] = dict(ms_per_step=am, frames_per_s=B * 1e3 / am, kernel_ms_in_step=ak,
                                                    frac_in_step=(n_kept * C * elem + n_int * 24 + B * D * H * W * C * 4) / (ak * 1e-3) / 8e12,
                                                    note="--overlap ahead with the bev_pool launch in front of the fork: nothing runs beside "
                                                         "the roofline kernel, the step pays for it (BEVAMD_BENCH_BEVPOOL_ALONE=1 makes it the "
                                                         "timed schedule)")
        except Exception as e:
            extra["fused_pool"] = dict(error=repr(e)[:300])
        # (i) BASELINE configs[1]: bev_pool on bf16 camera features, same plan, same launch
        if elem == 4:
            f16 = feats.bfloat16()
            km_b2b = kernel_ms(lambda: plan.launch_forward(f16, bev))
            km = kernel_duration_ms(lambda: plan.launch_forward(f16, bev))
            by = n_kept * C * 2 + n_int * 24 + B * D * H * W * C * 4
            extra["bev_pool_bf16_features"] = dict(kernel_ms=km, kernel_ms_back_to_back=km_b2b, algorithmic_bytes_per_launch=by,
                                                   achieved_gbs=by / (km * 1e-3) / 1e9, frac=by / (km * 1e-3) / 1e9 / HBM_PEAK_GBS, frames=B,
                                                   note="BASELINE configs[1]: bf16 features, fp32 accumulate / output; average duration of 20 "
                                                        "launches, one HIP event pair around each (kernel_ms_back_to_back: their rate without events)")
            del f16
        # (ii) the reference's own protocol is batch 1 (tools/benchmark.py:56-85): the same step on ONE frame
        try:
            per = geom.shape[0] // B
            plan1 = BevPoolPlan.from_geometry(geom[:per], 1, inp["origin"], inp["dx"], inp["nx"])
            plan1.prepare_fused(dbins, fh, fw, C)
            bev1, fused1 = torch.empty((1, D, H, W, C), device=dev), torch.empty((1, D, H, W, C), device=dev)
            feats1, depth1, ctx1, pts1 = feats[:per].float(), depth_prob[:n_cam], ctx_cl[: n_cam * fh * fw], pts_list[:1]

            def vox1():
                return voxelize_batch_device(pts1, cfg["voxel_size"], cfg["point_cloud_range"], cfg["max_num_points"],
                                             cfg["max_voxels"][1], order=args.voxel_order, encoder_rows=enc_rows)

            def enc1(vf, vc, _, cnt):
                with torch.no_grad():
                    return enc(vf, vc, 1, num_voxels=cnt, coors_order=coors_order)

            def geo1(vf, vc, _, cnt):
                with torch.no_grad():
                    return enc.prepare_geometry(vc, 1, num_voxels=cnt, coors_order=coors_order)

            def tail1(vf, vc, _, cnt, lvl):
                with torch.no_grad():
                    return enc(vf, vc, 1, num_voxels=cnt, geometry=lvl)

            for _ in range(2):
                enc1(*vox1())
            side1 = torch.cuda.Stream()
            side1.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side1):
                enc1(*vox1())
            torch.cuda.current_stream().wait_stream(side1)
            torch.cuda.synchronize()
            # the schedule of the headline step: voxelizer (own graph, second stream) beside raster + fused pooling, or one graph
            b1_voxel = overlap_voxel or overlap_lidar     # auto: a single frame runs the voxel schedule
            g1h = new_graph() if (b1_voxel or overlap_chain) else None
            g1g = new_graph() if overlap_chain else None
            g1 = new_graph()
            if overlap_chain:
                v1 = vox1()
                tail1(*v1, geo1(*v1))                       # eager once: the prepared-geometry route at one frame
                torch.cuda.synchronize()
                with torch.cuda.graph(g1h):
                    state["vox1"] = vox1()
                with torch.cuda.graph(g1g, pool=g1h.pool()):
                    state["geo1"] = geo1(*state["vox1"])
                with torch.cuda.graph(g1, pool=g1h.pool()):
                    state["lidar_bev1"] = tail1(*state["vox1"], state["geo1"])
            elif b1_voxel:
                with torch.cuda.graph(g1h):
                    state["vox1"] = vox1()
                with torch.cuda.graph(g1):
                    state["lidar_bev1"] = enc1(*state["vox1"])
            else:
                with torch.cuda.graph(g1):
                    state["lidar_bev1"] = enc1(*vox1())

            def step1():
                main_stream = torch.cuda.current_stream()
                if b1_voxel or overlap_chain:
                    head_stream.wait_stream(main_stream)
                    with torch.cuda.stream(head_stream):
                        g1h.replay()
                        if overlap_chain:
                            g1g.replay()          # one frame: the chain follows the voxelizer at once (both are short)
                with torch.no_grad():
                    vt.depth_raster(img_stub[:1], pts1, t_l2i[:1], t_ia[:1], t_la[:1])
                plan1.launch_fused(depth1.reshape(-1), ctx1, dbins, fh, fw, out=fused1)
                plan1.launch_forward(feats1, bev1)
                if b1_voxel or overlap_chain:
                    main_stream.wait_stream(head_stream)      # one frame: the join sits in front of the encoder (see early_join)
                g1.replay()

            def lidar1_alone():
                if b1_voxel or overlap_chain:
                    g1h.replay()
                if overlap_chain:
                    g1g.replay()
                g1.replay()

            m1 = timed(step1, 50, warm=5)
            ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            lidar1_alone()
            ev1[0].record()
            for _ in range(20):
                lidar1_alone()
            ev1[1].record()
            ev1[1].synchronize()
            extra["batch1_step"] = dict(ms_per_step=m1, frames_per_s=1e3 / m1, lidar_branch_ms=ev1[0].elapsed_time(ev1[1]) / 20,
                                        lidar_graph=(add_counts(graph_node_count(g1h), graph_node_count(g1)) if b1_voxel
                                                     else add_counts(add_counts(graph_node_count(g1h), graph_node_count(g1g)),
                                                                     graph_node_count(g1)) if overlap_chain else graph_node_count(g1)),
                                        note="the headline step (raster + fused pooling + bev_pool + LiDAR branch, same schedule) on "
                                             "ONE frame; lidar_branch_ms: voxelizer + encoder back to back, nothing beside them")
            del g1, g1h, g1g, plan1, bev1, fused1
        except Exception as e:   # a secondary figure must never take the headline down
            extra["batch1_step"] = dict(error=repr(e)[:300])
        # (iii) BASELINE configs[4]: 5 steps of the training step in the reference's default arithmetic, 4 frames
        try:
            import copy

            a2 = copy.copy(args)
            a2.amp, a2.steps, a2.warmup, a2.global_batch, a2.dump_outputs = True, 5, 2, 0, None
            tr = train_step(a2, 0, 1, list(range(4)), dev)
            extra["train_step_amp"] = dict(ms_per_step=tr["ms_per_step"], frames_per_s=tr["value"], frames=4, steps=5,
                                           stage_ms=tr["config"]["stage_ms"], bev_pool_bwd_frac=tr["roofline"]["frac"],
                                           plan_ms=tr["config"].get("plan_ms"), runs_per_column=tr["config"].get("runs_per_column"),
                                           fused_kernel=tr["config"].get("fused_kernel"), inputs=tr["config"].get("inputs"),
                                           bev_pool_bwd_kernel_ms=tr["roofline"]["kernel_ms"],
                                           note="--mode train-step --amp (fp16 conv operands, fp32 accumulate / master weights): fwd + "
                                                "bwd + clip + AdamW of bev_pool, fused pooling, voxelize, SparseEncoder at 4 frames")
        except Exception as e:
            extra["train_step_amp"] = dict(error=repr(e)[:300])
        extra["wall_s"] = time.perf_counter() - t_extra
    per_rank = [dict(rank=rank, frames=B, ms_per_step=elapsed_local / args.steps * 1e3,
                     frames_per_s=B * args.steps / elapsed_local, cpu_binding=args.cpu_binding)]
    if world > 1:
        import torch.distributed as dist

        gathered = [None] * world
        dist.all_gather_object(gathered, per_rank[0])
        per_rank = gathered

    if rank == 0:
        frames = args.steps * frames_per_step
        # algorithmic bytes of the bev_pool scatter: every kept feature row read once + one
        # (geom, start, length) record per interval + every output cell written once
        alg_bytes = n_kept * C * elem + n_int * 24 + B * D * H * W * C * 4
        roof_ms = solo_ms if solo_ms is not None else kern_ms
        achieved = alg_bytes / (roof_ms * 1e-3) / 1e9
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "bev_pool_traffic.json")
        if os.path.exists(tpath):
            try:
                # PMC figure of tools/pmc_bev_pool.sh, per frame x frames per launch (the traffic is linear in the frames)
                traffic = json.load(open(tpath)).get("hbm_bytes_per_frame") * B
            except Exception:
                traffic = None
        rocprof_us = rocprof_src = None
        rpath = os.path.join(ROOT, "profiles", "roofline_rocprof.json")
        if os.path.exists(rpath):
            try:
                rj = json.load(open(rpath))
                rocprof_us, rocprof_src = rj.get("solo_avg_us"), f"profiles/roofline_rocprof.json (round {rj.get('round')}, stored: {rj.get('source')})"
            except Exception:
                pass
        res = {
            "metric": "frames/sec of the BEVFusion C+L hot path (6x256x704 cameras -> 360x360/180x180 BEV, ~310k LiDAR "
                      "points); bev_pool HBM GB/s in roofline",
            "value": frames / elapsed,
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "ms_per_frame": elapsed / args.steps * 1e3 / B,
            "higher_is_better": True,
            "scaling": "strong" if args.global_batch else "weak",
            "vs_baseline": None,
            "dtype": f"f32 (bev_pool acc, voxelize) + {args.spconv_dtype}/f32-acc (sparse conv)"
                     + ("" if elem == 4 else ", bf16 camera features"),
            "data": "synthetic",
            "config": {
                "workload": "hot path of the C+L model (BASELINE configs[1]+[2]: camera view-transform reduction and LiDAR "
                            f"voxel pipeline) at {B} frame(s)/step/GPU (configs[3] quotes batch 8): bev_pool N'={geom.shape[0]} frustum points ({n_kept} kept) "
                            f"x C={C} -> {n_int} non-empty of {B * D * H * W} cells; hard voxelize {sum(p.shape[0] for p in pts_all)} points -> "
                            f"{state['n_voxels']} voxels; SparseEncoder 1440x1440x41 (17 SubM + 4 strided convs) -> "
                            f"[{B},256,180,180]. bev_pool rank/sort/CSR precompute cached per calibration.",
                "frames_per_step_per_gpu": B,
                "frames_per_step": frames_per_step,
                "inputs": "synthetic, resident in HBM; ONE calibration shared by all frames and ranks, camera rig without pitch/roll "
                          "(the easy case of the column pooling: extra.fused_pool_rigged_ms times a pitched/rolled rig), "
                          + ("two sets of point clouds alternating from step to step (graph replay on two sets of static buffers)" if overlap_ahead
                             else "the same point clouds every step (graph replay on static buffers)"),
                "host_gc": "Python's cyclic collector is off inside the timed region (timeit's convention; see quiet_gc)",
                "parallelism": f"frames sharded over {world} rank(s), one process per GPU, no data-path collective"
                               + (f"; torch.distributed backend nccl (= RCCL) world size {world}" if world > 1 else ""),
                "per_rank": per_rank,
                "rccl_ranks": rccl_ranks,
                "stages": STAGES,
                "stage_ms": dict(zip(["depth_raster", "fused_depth_context_pool", "bev_pool", "lidar_branch"], stage_ms)),
                "camera_branch": {
                    "starts_from": "depth distribution [B*6,118,32,88] + context [B*6*32*88,80] + LiDAR points + calibration",
                    "depth_raster_ms": stage_ms[0], "fused_pool_ms": stage_ms[1],
                    "geometry_and_plan_ms_uncached": geometry_plan_ms,
                    "note": "geometry + pooling plan are cached per calibration at inference and are NOT in the step; the "
                            "materialised-volume bev_pool stage is the API-level op of the HBM GB/s metric and is in the step "
                            "too, so the camera reduction is counted twice in `value`"},
                "lidar_branch_eager_ms": {"voxelize": eager_vox_ms, "sparse_encoder": eager_enc_ms},
                "hip_graph": graph is not None or graph_tail is not None or ahead_sets is not None,
                "voxel_order": args.voxel_order,
                "overlap": ("ahead: software pipeline across steps, two alternating buffer sets (own point clouds). Step t = camera stages of "
                            "batch t + its 21 convolutions and dense tail (2nd HIP stream; rulebooks built in step t-1) + voxelizer and rulebook "
                            "chain of batch t+1 (3rd stream, started "
                            + {"fused": "behind the fused pooling", "bev_pool": "behind bev_pool"}.get(ahead_gate, "with the step")
                            + "), joined at the end: batch t is complete when step t ends; every step pays one head + one tail "
                            "(extra.unpipelined_step_ms: head inside its own step). stage_ms.bev_pool: the kernel WITH the rest beside it") if overlap_ahead else
                           ("chain: voxelizer graph on a second HIP stream beside depth raster + fused pooling, the encoder's rulebook-chain graph "
                            "on that stream beside bev_pool" + (" (gated: it starts when the fused pooling has finished)" if chain_gate else "")
                            + ", join, then the 21 convolutions + dense tail alone; stage_ms.bev_pool is the kernel WITH the chain beside it, "
                            "roofline.kernel_ms the same launch SOLO after the timed region") if overlap_chain else
                           ("pipeline: bev_pool first with the voxelizer beside it (second HIP stream), then depth raster + fused pooling with "
                            "the rulebook chain beside them, then the convolutions alone (stage_ms in the canonical order; `stages` names "
                            "the execution order)") if overlap_pipe else
                           ("voxel: the voxelizer on a second HIP stream beside the depth raster / fused pooling stages; "
                            + ("the join sits in front of bev_pool, which runs alone; " if early_join else
                               "the join sits in front of the encoder (1-3 frames per step: the voxelizer outlasts the two camera stages); ")
                            + "the encoder, rulebook chain included, follows") if overlap_voxel else
                           ("head: voxelization + rulebook chain on a second HIP stream beside the camera stages (the camera stage times, "
                            "bev_pool's roofline figure included, are measured WITH that concurrency)") if overlap_head else
                           ("lidar: the whole LiDAR branch (one HIP graph: voxelizer, rulebook chain, convolutions) on a second HIP stream beside "
                            "the camera stages; stage times overlap (the last stage is the wait for the branch), stage_ms.bev_pool is the kernel "
                            "WITH the branch beside it, roofline.kernel_ms the same launch SOLO right after the timed region")
                           if overlap_lidar else "none",
                "fused_depth_context_bev": {"ms": fused_ms, "algorithmic_bytes": fused_bytes,
                                            "gbs_on_own_bytes": fused_bytes / (fused_ms * 1e-3) / 1e9,
                                            "note": "stage of the step: out[cell] = sum depth*ctx straight from depth "
                                                    "[6,118,32,88] + context [6*32*88,80] (the [N',80] volume never exists); "
                                                    "L2-bound, own byte denominator (SURVEY.md 8d/8f), not comparable with the "
                                                    "bev_pool roofline figure"},
                "bev_pool_precompute_ms_uncached": precompute_ms,
                "bev_pool_precompute_first_call_ms": t_first * 1e3,
            },
            "extra": extra,
            "roofline_spconv": roofline_spconv,
            "roofline": {
                "kernel": "bev_pool_fwd_cells_vec_kernel",
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic,
                "traffic_source": "profiles/bev_pool_traffic.json (FETCH_SIZE x2 + WRITE_SIZE from two separate rocprofv3 --pmc "
                                  "passes of tools/pmc_bev_pool.sh, per frame x frames per launch) — not measured inside this run",
                "algorithmic_bytes_per_launch": alg_bytes,
                "kernel_ms": roof_ms,
                "kernel_ms_back_to_back": solo_b2b_ms,
                "rocprof_kernel_us": rocprof_us,
                "rocprof_source": rocprof_src,
                "kernel_ms_in_step": kern_ms,
                "frac_in_step": alg_bytes / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "measured": ("solo: mean duration of 20 launches after the timed region, one HIP event pair around EACH (as a kernel "
                             "trace measures; rocprof_kernel_us: the stored trace); kernel_ms_in_step: with the LiDAR streams beside it "
                             "(extra.alone_frac_in_step: first and alone in the step)") if solo_ms is not None else
                            ("in the step: HIP events around the one launch of every timed step, with the LiDAR streams beside it "
                             "(--full adds the solo figure)") if shared else
                            "in the step: HIP events around the one launch of every timed step, nothing beside it",
            },
        }
        bf = (extra or {}).get("bev_pool_bf16_features")
        if bf and "frac" in bf:      # full file only: the same kernel on bf16 features = BASELINE configs[1]
            res["roofline_bf16"] = {"kernel": "bev_pool_fwd_cells_vec_kernel<U4, 8, 4, 0, true, 1> (bf16 features, fp32 accumulate)",
                                    "bound": "hbm", "achieved": bf["achieved_gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bf["frac"],
                                    "traffic": None, "algorithmic_bytes_per_launch": bf["algorithmic_bytes_per_launch"],
                                    "kernel_ms": bf["kernel_ms"], "kernel_ms_back_to_back": bf.get("kernel_ms_back_to_back"),
                                    "measured": "solo, right after the timed region: average duration of 20 launches, one HIP event pair around each"}
        res["box"] = box_sampled
        if cpu_base:
            res["cpu_baseline"] = cpu_baseline(inp, pts_np, cfg, B, D, H, W)
        else:
            res["cpu_baseline"] = None
        emit(res)

    if world > 1:
        import torch.distributed as dist

        dist.destroy_process_group()


if __name__ == "__main__":
    main()
