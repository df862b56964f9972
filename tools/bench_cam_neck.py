"""Times the camera necks' eval-mode forward on an MI355X in fp16, at B = 1 and B = 8 frames:

  gen_swint  GeneralizedLSSFPN [192, 384, 768] -> 256 on 6 cameras a frame at 256 x 704 (maps 32 x 88, 16 x 44, 8 x 22);
  lssfpn     LSSFPN in_channels [640, 160] -> 256, scale_factor 2 (640 channels on 90 x 90 resampled to 180 x 180, output 360 x 360);
  layers     the layer classes on their own: the two resampling 1x1 layers of gen_swint, LSSFPN's resampling 1x1 layer and its
             upsampling 3x3 layer, each as one `cam_neck_conv_forward` against the torch layers it replaces (F.interpolate, cat,
             convolution, BatchNorm, ReLU),

as (i) the fused path (two launches a level, no upsampled tensor, no `cat`) and (ii) the module's own torch layers in the same dtype
with `use_fused = False`, in contiguous NCHW and in channels-last, with the backend's benchmark mode on; the faster of the two torch
formats is the comparison.

Device events around `--iters` calls after `--warmup` calls, the paths alternating inside every round; the median round is reported
with the spread.  The MFMA floor 2 * MAC / 2.5 PFLOP/s is printed beside the times.

Every step runs in a child process of its own under `timeout`; a step that fails, faults or runs out of time ends the run and
nothing further is started on the GPU.

    python tools/bench_cam_neck.py [--iters 20] [--warmup 3] [--rounds 5] [--json profiles/cam_neck_timing.json]
"""
import argparse
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_bev_trunk import PEAK_FP16_MATRIX, compare, randomise  # noqa: E402

FRAMES = (1, 8)
STEP_SECONDS = {"gen_swint": 300, "lssfpn": 300, "layers": 300}
SWINT = [(192, (32, 88)), (384, (16, 44)), (768, (8, 22))]
LSS = [(160, (180, 180)), (640, (90, 90))]


def inputs(shapes, n, dev, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    return [torch.randn((n, c) + hw, generator=g).half().to(dev) for c, hw in shapes]


def conv_macs(module, xs):
    """Multiply-accumulates of one forward of the torch layers, from the convolutions' shapes."""
    import torch

    total, hooks = 0, []

    def hook(m, args, out):
        nonlocal total
        total += out.shape[0] * out.shape[2] * out.shape[3] * m.in_channels * m.out_channels * m.kernel_size[0] * m.kernel_size[1]
    for m in module.modules():
        if isinstance(m, torch.nn.Conv2d):
            hooks.append(m.register_forward_hook(hook))
    was, module.use_fused = module.use_fused, False
    with torch.no_grad():
        module(xs)
    module.use_fused = was
    for h in hooks:
        h.remove()
    return total


def last(y):
    return y[0] if isinstance(y, (tuple, list)) else y


def entry(med, spread, mac, err):
    best = min(med["torch_nchw"], med["torch_nhwc"])
    return dict(ms=med, spread=spread, mac=mac, floor_ms=2 * mac / PEAK_FP16_MATRIX * 1e3, torch_best_ms=best,
                fused_TFLOPs=2 * mac / (med["fused"] * 1e-3) / 1e12, speedup=best / med["fused"], max_rel_diff=err)


def measure_module(make, shapes, images_per_frame, args, dev, seed):
    import torch

    torch.backends.cudnn.benchmark = True
    mod = randomise(make(), seed).to(dev).half().eval()
    twin = copy.deepcopy(mod).to(memory_format=torch.channels_last)
    mod.use_fused, twin.use_fused = True, False
    plain = copy.deepcopy(mod)
    plain.use_fused = False
    out = {}
    with torch.no_grad():
        for B in FRAMES:
            xs = inputs(shapes, B * images_per_frame, dev, seed + B)
            xc = [x.contiguous(memory_format=torch.channels_last) for x in xs]
            assert mod.fusable(xs) and not plain.fusable(xs)
            ref, got = last(plain(xs)).float(), last(mod(xs)).float()
            err = float((got - ref).abs().max()) / float(ref.abs().max())
            assert err < 2e-2, err                      # both paths compute the same layers (fp16 storage)
            paths = {"fused": lambda: mod(xs), "torch_nchw": lambda: plain(xs), "torch_nhwc": lambda: twin(xc)}
            med, spread = compare(paths, args.iters, args.warmup, args.rounds)
            out[f"B{B}"] = entry(med, spread, conv_macs(plain, xs), err)
    return out


def step_gen_swint(args):
    import torch

    from bevfusion_amd import cam_neck as cnk
    return measure_module(lambda: cnk.GeneralizedLSSFPN([c for c, _ in SWINT], 256, 3), SWINT, 6, args, torch.device("cuda:0"), 1)


def step_lssfpn(args):
    import torch

    from bevfusion_amd import cam_neck as cnk
    return measure_module(lambda: cnk.LSSFPN([-1, 0], [640, 160], 256, scale_factor=2), LSS, 1, args, torch.device("cuda:0"), 2)


def step_layers(args):
    """One resampling layer at a time: (name, [(channels, map)] in cat order, output map, kernel, images per frame)."""
    import torch
    import torch.nn.functional as F
    from torch import nn

    from bevfusion_amd import cam_neck as cnk

    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = True
    layers = [("gen_lateral_16x44", [(384, (16, 44)), (768, (8, 22))], (16, 44), 1, 6),
              ("gen_lateral_32x88", [(192, (32, 88)), (256, (16, 44))], (32, 88), 1, 6),
              ("lss_fuse_180x180", [(640, (90, 90)), (160, (180, 180))], (180, 180), 1, 1),
              ("lss_upsample_360x360", [(256, (180, 180))], (360, 360), 3, 1)]
    out = {}
    with torch.no_grad():
        for i, (name, shapes, size, k, per_frame) in enumerate(layers):
            seq = randomise(nn.Sequential(nn.Conv2d(sum(c for c, _ in shapes), 256, k, padding=k // 2, bias=False), nn.BatchNorm2d(256),
                                          nn.ReLU(True)), 10 + i).to(dev).half().eval()
            seq_cl = copy.deepcopy(seq).to(memory_format=torch.channels_last)
            fold = cnk.fold_neck_layer(seq[0], seq[1])
            out[name] = {}
            for B in FRAMES:
                xs = inputs(shapes, B * per_frame, dev, 20 + i + B)
                # the fused path's sources as the modules hand them over: backbone maps NCHW, a fused layer's output channels-last
                xf = [x.contiguous(memory_format=torch.channels_last) if c == 256 else x for x, (c, _) in zip(xs, shapes)]
                xc = [x.contiguous(memory_format=torch.channels_last) for x in xs]

                def torch_path(s, ts):
                    ts = [t if tuple(t.shape[2:]) == size else F.interpolate(t, size=size, mode="bilinear", align_corners=True) for t in ts]
                    return s(torch.cat(ts, dim=1) if len(ts) > 1 else ts[0])
                paths = {"fused": lambda: cnk.cam_neck_conv_forward(xf, fold, out_size=size),
                         "torch_nchw": lambda: torch_path(seq, xs), "torch_nhwc": lambda: torch_path(seq_cl, xc)}
                ref, got = paths["torch_nchw"]().float(), paths["fused"]().float()
                err = float((got - ref).abs().max()) / float(ref.abs().max())
                assert err < 2e-2, err
                med, spread = compare(paths, args.iters, args.warmup, args.rounds)
                mac = xs[0].shape[0] * size[0] * size[1] * seq[0].in_channels * 256 * k * k
                out[name][f"B{B}"] = entry(med, spread, mac, err)
    return out


STEPS = {"gen_swint": step_gen_swint, "lssfpn": step_lssfpn, "layers": step_layers}


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
            raise SystemExit("bench_cam_neck needs a GPU: nothing is measured without one")
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
