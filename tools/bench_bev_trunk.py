"""Times the dense BEV trunk's eval-mode forward on an MI355X at the flagship widths (ConvFuser [80, 256] -> 256, SECOND 256 ->
[128, 256] with layer_nums [5, 5] and strides [1, 2], SECONDFPN [128, 256] -> [256, 256] with strides [1, 2] and
use_conv_for_no_stride) on a 180 x 180 map, at B = 1 and B = 8, in fp16:

  layers   one layer of every class (336 -> 256 with its two sources; 128 -> 128; the stride-2 layer 128 -> 256; 256 -> 256 on
           90 x 90; the neck with both levels) as (i) the fused kernel (`bevamd_bev_conv_forward`, one launch per layer, no `cat`) and
           (ii) the module's torch layers in the same dtype with `use_fused = False`, in contiguous NCHW and in channels-last, with
           the backend's benchmark mode on; the faster of the two torch formats is the comparison;
  trunk    the three modules in a row, the same three paths; "fused" is the modules' default choice of layer classes
           (`SECOND.fused_stride2`), "fused_all" every layer through the kernel.

Device events around `--iters` calls after `--warmup` calls, the paths alternating inside every round; the median round is reported
with the spread.  The MFMA floor 2 * MAC / 2.5 PFLOP/s is printed beside the times.

Every step runs in a child process of its own under `timeout`; a step that fails, faults or runs out of time ends the run and
nothing further is started on the GPU.

    python tools/bench_bev_trunk.py [--iters 20] [--warmup 3] [--rounds 5] [--json profiles/bev_trunk_timing.json]
"""
import argparse
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAP, BATCHES = 180, (1, 8)
PEAK_FP16_MATRIX = 2.5e15
STEP_SECONDS = {"layers": 420, "trunk": 420}


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
    """Weights of variance 2 / K and BatchNorm statistics that are not the defaults."""
    import torch

    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                K = m.in_channels * (m.kernel_size[0] * m.kernel_size[1] if isinstance(m, torch.nn.Conv2d) else 1)
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / K) ** 0.5)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(0.8 + 0.4 * torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.num_features, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(m.num_features, generator=g))
    return module


def macs(module, inputs):
    """Multiply-accumulates of one forward, from the layers' shapes."""
    import torch

    total = 0
    hooks = []

    def hook(m, args, out):
        nonlocal total
        k = m.kernel_size[0] * m.kernel_size[1]
        if isinstance(m, torch.nn.ConvTranspose2d):
            total += args[0].shape[0] * args[0].shape[2] * args[0].shape[3] * m.in_channels * m.out_channels * k
        else:
            total += out.shape[0] * out.shape[2] * out.shape[3] * m.in_channels * m.out_channels * k
    for m in module.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            hooks.append(m.register_forward_hook(hook))
    was = [getattr(m, "use_fused", None) for m in module]
    for m in module:
        m.use_fused = False
    with torch.no_grad():
        run(module, inputs)
    for m, w in zip(module, was):
        m.use_fused = w
    for h in hooks:
        h.remove()
    return total


def run(mods, inputs):
    """mods: a ModuleList chained as fuser -> backbone -> neck where present; inputs: what the first one takes."""
    x = inputs
    for m in mods:
        x = m(x)
    return x


def classes(dev):
    """name -> (ModuleList, input builder(B, channels_last))"""
    import torch
    from torch import nn

    from bevfusion_amd import bev_trunk as bt

    def maps(shapes, seed):
        def make(B, cl):
            g = torch.Generator().manual_seed(seed + B)
            ts = [torch.randn((B,) + s, generator=g).half().to(dev) for s in shapes]
            return [t.contiguous(memory_format=torch.channels_last) if cl else t for t in ts]
        return make

    def one(shape, seed):
        make = maps([shape], seed)
        return lambda B, cl: make(B, cl)[0]
    h = MAP // 2
    out = {
        "fuser_336_256": (nn.ModuleList([bt.ConvFuser([80, 256], 256)]), maps([(80, MAP, MAP), (256, MAP, MAP)], 1)),
        "conv_128_128": (nn.ModuleList([bt.SECOND(128, [128], [0], [1])]), one((128, MAP, MAP), 2)),
        "conv_128_256_s2": (nn.ModuleList([bt.SECOND(128, [256], [0], [2])]), one((128, MAP, MAP), 3)),
        "conv_256_256": (nn.ModuleList([bt.SECOND(256, [256], [0], [1])]), one((256, h, h), 4)),
        "neck": (nn.ModuleList([bt.SECONDFPN([128, 256], [256, 256], [1, 2], use_conv_for_no_stride=True)]), maps([(128, MAP, MAP), (256, h, h)], 5)),
    }
    trunk = nn.ModuleList([bt.ConvFuser([80, 256], 256), bt.SECOND(256, [128, 256], [5, 5], [1, 2]), bt.SECONDFPN([128, 256], [256, 256], [1, 2], use_conv_for_no_stride=True)])
    return out, (trunk, maps([(80, MAP, MAP), (256, MAP, MAP)], 6))


def first(y):
    while isinstance(y, (list, tuple)):
        y = y[-1]
    return y


def measure(mods, make, fused_channels_last, args, dev, per_class=True):
    """per_class: every layer through the kernel ("fused").  Otherwise "fused" is the modules' default choice of layer classes
    (`SECOND.fused_stride2`) and "fused_all" every layer through the kernel."""
    import torch

    defaults = [getattr(m, "fused_stride2", None) for m in mods]
    torch.backends.cudnn.benchmark = True
    randomise(mods, 7)
    mods.to(dev).half().eval()
    twin = copy.deepcopy(mods).to(memory_format=torch.channels_last)
    out = {}
    with torch.no_grad():
        for B in BATCHES:
            x_f, x_n, x_c = make(B, fused_channels_last), make(B, False), make(B, True)

            def fused_all():
                for m in mods:
                    m.use_fused = True
                    if hasattr(m, "fused_stride2"):
                        m.fused_stride2 = True
                return run(mods, x_f)

            def fused_default():
                for m, d in zip(mods, defaults):
                    m.use_fused = True
                    if hasattr(m, "fused_stride2"):
                        m.fused_stride2 = d
                return run(mods, x_f)

            fused = fused_all if per_class else fused_default

            def torch_nchw():
                for m in mods:
                    m.use_fused = False
                return run(mods, x_n)

            def torch_nhwc():
                for m in twin:
                    m.use_fused = False
                return run(twin, x_c)

            for m in mods:
                m.use_fused = True
                if per_class and hasattr(m, "fused_stride2"):
                    m.fused_stride2 = True
            assert mods[0].fusable(x_f)
            ref, got = first(torch_nchw()).float(), first(fused()).float()
            err = float((got - ref).abs().max()) / float(ref.abs().max())
            assert err < 2e-2, err                      # both paths compute the same layers (fp16 storage)
            paths = {"fused": fused, "torch_nchw": torch_nchw, "torch_nhwc": torch_nhwc}
            if not per_class:
                paths["fused_all"] = fused_all
            med, spread = compare(paths, args.iters, args.warmup, args.rounds)
            mac = macs(mods, x_n)
            best = min(med["torch_nchw"], med["torch_nhwc"])
            out[f"B{B}"] = dict(ms=med, spread=spread, mac=mac, floor_ms=2 * mac / PEAK_FP16_MATRIX * 1e3, torch_best_ms=best,
                                fused_TFLOPs=2 * mac / (med["fused"] * 1e-3) / 1e12, speedup=best / med["fused"], max_rel_diff=err)
    return out


def step_layers(args):
    import torch

    dev = torch.device("cuda:0")
    per_class, _ = classes(dev)
    return {name: measure(mods, make, name != "fuser_336_256", args, dev) for name, (mods, make) in per_class.items()}


def step_trunk(args):
    import torch

    dev = torch.device("cuda:0")
    _, (trunk, make) = classes(dev)
    return measure(trunk, make, False, args, dev, per_class=False)


STEPS = {"layers": step_layers, "trunk": step_trunk}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_bev_trunk needs a GPU: nothing is measured without one")
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
