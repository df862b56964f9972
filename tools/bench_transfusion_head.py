"""Times TransFusionHead's eval-mode forward on an MI355X at the config shape (hidden 128, 10 classes, 200 proposals, the YAML's six
prediction heads):

  heads    the prediction heads of one decoder layer with `+ query_pos` on the center head, and the category encoding, each as
           (i) this module's torch path, which is the reference's formulation op for op (per head Conv1d -> BatchNorm1d -> ReLU ->
           Conv1d, then the add; one_hot -> permute -> float -> Conv1d -> add), and (ii) the fused kernel (`bevamd_head_ffn_forward`,
           `bevamd_head_class_encoding`), at B = 1 and B = 8 with P = 200;
  forward  the whole `forward` on a [B, 512, 180, 180] BEV map at B = 1, `use_fused` False against True.

Device events around `--iters` calls after `--warmup` calls, the two paths alternating inside every round; the median round is
reported with the spread.  Both paths are compared on the timed inputs before anything is timed.

Every step runs in a child process of its own under `timeout`; a step that fails, faults or runs out of time ends the run and
nothing further is started on the GPU.

    python tools/bench_transfusion_head.py [--iters 500] [--warmup 20] [--rounds 7] [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS = dict(center=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2), heatmap=(10, 2))
HIDDEN, CLASSES, PROPOSALS, IN_CHANNELS, BEV = 128, 10, 200, 512, 180
STEP_SECONDS = {"heads": 240, "forward": 300}


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


def step_heads(args):
    import torch
    import torch.nn.functional as F

    from bevfusion_amd import transfusion_head as th

    dev = torch.device("cuda:0")
    ffn = th.FFN(HIDDEN, dict(HEADS), head_conv=64)
    randomise(ffn, 1)
    ffn = ffn.to(dev).eval()
    enc = torch.nn.Conv1d(CLASSES, HIDDEN, 1).to(dev)
    out = {}
    with torch.no_grad():
        for B in (1, 8):
            gen = torch.Generator().manual_seed(B)
            x = torch.randn((B, HIDDEN, PROPOSALS), generator=gen).to(dev)
            qpos = (torch.rand((B, PROPOSALS, 2), generator=gen) * BEV).to(dev)
            labels = torch.randint(0, CLASSES, (B, PROPOSALS), generator=gen).to(dev)
            qfeat = torch.randn((B, HIDDEN, PROPOSALS), generator=gen).to(dev)

            def heads_path(fused):
                ffn.use_fused = fused
                return ffn(x, qpos)

            def encoding_torch():
                one_hot = F.one_hot(labels, num_classes=CLASSES).permute(0, 2, 1)
                q = qfeat.clone()
                q += enc(one_hot.float())
                return q

            def encoding_fused():
                return th.head_class_encoding(qfeat.clone(), labels, enc.weight, enc.bias)

            assert ffn.fusable(x)
            ref, got = heads_path(False), heads_path(True)
            for name in HEADS:
                err = float((got[name] - ref[name]).abs().max()) / float(ref[name].abs().max())
                assert err < 1e-5, (name, err)            # both paths compute the same heads
            assert torch.equal(encoding_torch(), encoding_fused())
            paths = {"heads_torch": lambda: heads_path(False), "heads_fused": lambda: heads_path(True),
                     "encoding_torch": encoding_torch, "encoding_fused": encoding_fused}
            med, spread = compare(paths, args.iters, args.warmup, args.rounds)
            flop = 2 * B * PROPOSALS * sum(HIDDEN * 64 + 64 * c for c, _ in HEADS.values())
            out[f"B{B}"] = dict(ms=med, spread=spread, heads_flop=flop, heads_fused_GFLOPs=flop / (med["heads_fused"] * 1e-3) / 1e9)
    return out


def step_forward(args):
    import torch

    from bevfusion_amd import transfusion_head as th

    dev = torch.device("cuda:0")
    head = th.TransFusionHead(
        num_proposals=PROPOSALS, auxiliary=True, in_channels=IN_CHANNELS, hidden_channel=HIDDEN, num_classes=CLASSES, num_decoder_layers=1,
        num_heads=8, nms_kernel_size=3, ffn_channel=256, common_heads={k: v for k, v in HEADS.items() if k != "heatmap"},
        loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0),
        test_cfg=dict(dataset="nuScenes", grid_size=[BEV * 8, BEV * 8, 41], out_size_factor=8, voxel_size=[0.075, 0.075],
                      pc_range=[-54.0, -54.0], nms_type=None))
    randomise(head, 2)
    head = head.to(dev).eval()
    x = torch.randn((1, IN_CHANNELS, BEV, BEV), generator=torch.Generator().manual_seed(3)).to(dev)

    def run(fused):
        head.use_fused = fused
        return head(x)[0][0]

    with torch.no_grad():
        ref, got = run(False), run(True)
        for key in ref:
            err = float((got[key] - ref[key]).abs().max()) / float(ref[key].abs().max())
            assert err < 1e-5, (key, err)
        iters = max(args.iters // 10, 10)
        med, spread = compare({"forward_torch": lambda: run(False), "forward_fused": lambda: run(True)}, iters, max(args.warmup // 2, 3),
                              args.rounds)
    return dict(B1=dict(ms=med, spread=spread, iters=iters))


STEPS = {"heads": step_heads, "forward": step_forward}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_transfusion_head needs a GPU: nothing is measured without one")
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
