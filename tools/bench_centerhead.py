"""Times CenterHead's eval-mode forward on an MI355X at the config shape (`configs/nuscenes/det/centerhead`: 6 tasks of 6 heads,
share_conv_channel 64, final_kernel 3, in_channels 256) on a 128 x 128 map, at B = 1 and B = 4:

  heads    the 36 task-head stacks on the shared map as (i) this module's torch layers with `use_fused = False`, which is the
           reference's formulation op for op (per head Conv2d -> BatchNorm2d -> ReLU -> Conv2d: 144 launches) and is what exists
           without the kernel, and (ii) the fused kernel (`bevamd_center_heads_forward`, one launch);
  forward  the whole `forward` (shared_conv, then the task heads), `use_fused` False against True.

Device events around `--iters` calls after `--warmup` calls, the two paths alternating inside every round; the median round is
reported with the spread.  Both paths are compared on the timed inputs before anything is timed.  The fused heads are reported next
to the arithmetic floor of the issue: 36 x (2 * 64 * 64 * 9) + 70 x (2 * 64 * 9) FLOP per cell at 157 TFLOP/s.

Every step runs in a child process of its own under `timeout`; a step that fails, faults or runs out of time ends the run and
nothing further is started on the GPU.

    python tools/bench_centerhead.py [--iters 200] [--warmup 10] [--rounds 7] [--json profiles/centerhead_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASKS = [["car"], ["truck", "construction_vehicle"], ["bus", "trailer"], ["barrier"], ["motorcycle", "bicycle"], ["pedestrian", "traffic_cone"]]
COMMON_HEADS = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
IN_CHANNELS, SHARED, MAP, BATCHES = 256, 64, 128, (1, 4)
PEAK_FP32_MATRIX = 157e12
STEP_SECONDS = {"heads": 300, "forward": 300}


def timed(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def compare(paths, iters, warmup, rounds):
    """{name: fn} -> {name: median ms}, {name: [min, max]}; the paths alternate inside every round."""
    import torch

    for fn in paths.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            ms[k].append(timed(fn, iters))
    return {k: sorted(v)[len(v) // 2] for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}


def randomise(module, seed):
    """Non-trivial parameters and BatchNorm statistics from a seed."""
    import torch

    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if name.endswith("running_var"):
                t.copy_(torch.rand(t.shape, generator=gen) * 1.5 + 0.5)
            elif name.endswith("running_mean"):
                t.copy_(torch.rand(t.shape, generator=gen) - 0.5)
            elif t.dtype.is_floating_point and t.dim() == 1:
                t.copy_(torch.rand(t.shape, generator=gen) * 0.4 + (0.8 if name.endswith("weight") else -0.2))


def make_head(dev):
    from bevfusion_amd import centerhead_module as cm

    head = cm.CenterHead(in_channels=IN_CHANNELS, tasks=[list(t) for t in TASKS], common_heads=dict(COMMON_HEADS), share_conv_channel=SHARED,
                         separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3))
    randomise(head, 1)
    return head.to(dev).eval()


def same(ref, got):
    for r, g in zip(ref, got):
        for name in r:
            err = float((g[name] - r[name]).abs().max()) / float(r[name].abs().max())
            assert err < 1e-5, (name, err)            # both paths compute the same heads


def floor_ms(B):
    channels = sum(c for c, _ in COMMON_HEADS.values()) * len(TASKS) + sum(len(t) for t in TASKS)
    flop = B * MAP * MAP * (len(TASKS) * (len(COMMON_HEADS) + 1) * 2 * SHARED * SHARED * 9 + channels * 2 * SHARED * 9)
    return flop, flop / PEAK_FP32_MATRIX * 1e3


def step_heads(args):
    import torch

    from bevfusion_amd import centerhead_module as cm

    dev = torch.device("cuda:0")
    head = make_head(dev)
    out = {}
    with torch.no_grad():
        folded = head.folded()
        for B in BATCHES:
            x = torch.randn((B, SHARED, MAP, MAP), generator=torch.Generator().manual_seed(B)).to(dev)

            def torch_path():
                return [task(x) for task in head.task_heads]

            def fused_path():
                res = cm.center_heads_forward(x, folded)
                return [dict(zip(task.heads, r)) for task, r in zip(head.task_heads, res)]

            head.use_fused = False
            assert not head.task_heads[0].fusable(x)
            same(torch_path(), fused_path())
            med, spread = compare({"heads_torch": torch_path, "heads_fused": fused_path}, args.iters, args.warmup, args.rounds)
            flop, floor = floor_ms(B)
            out[f"B{B}"] = dict(ms=med, spread=spread, heads_flop=flop, floor_ms=floor, heads_fused_TFLOPs=flop / (med["heads_fused"] * 1e-3) / 1e12,
                                speedup=med["heads_torch"] / med["heads_fused"])
    return out


def step_forward(args):
    import torch

    dev = torch.device("cuda:0")
    head = make_head(dev)
    out = {}
    with torch.no_grad():
        for B in BATCHES:
            x = torch.randn((B, IN_CHANNELS, MAP, MAP), generator=torch.Generator().manual_seed(10 + B)).to(dev)

            def run(fused):
                head.use_fused = fused
                return head.forward_single(x)

            head.use_fused = True
            assert head.fusable(x)
            same(run(False), run(True))
            med, spread = compare({"forward_torch": lambda: run(False), "forward_fused": lambda: run(True)}, args.iters, args.warmup,
                                  args.rounds)
            out[f"B{B}"] = dict(ms=med, spread=spread, speedup=med["forward_torch"] / med["forward_fused"])
    return out


STEPS = {"heads": step_heads, "forward": step_forward}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_centerhead needs a GPU: nothing is measured without one")
        print("RESULT " + json.dumps(STEPS[args.step](args)), flush=True)
        return
    results = {}
    for step, seconds in STEP_SECONDS.items():
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(args.iters),
               "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"step {step} ended with status {r.returncode}: nothing further is started")
        results[step] = json.loads(lines[-1][len("RESULT "):])
        print(f"{step}: {lines[-1][len('RESULT '):]}", file=sys.stderr, flush=True)
    line = json.dumps(results)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
