"""Times the pillar / radar feature nets + scatter on an MI355X at the configs' max_voxels (60 000 radar pillars, 30 000 LiDAR
pillars, P = 20, num_points uniform in 1..P):

  (i)   the reference's formulation in plain torch ops on the GPU (decorations by slicing and cat, the layer loop, the per-sample
        scatter loop) — the yardstick;
  (ii)  this package's unfused path (decorate kernel + the module's torch layers + the scatter kernels);
  (iii) the fused stack + the scatter kernels (the default dispatch in eval mode).

Device events around `--iters` calls after `--warmup` calls, (i)/(ii)/(iii) alternating inside every round; the median round is
reported.  The fused kernel's own time (feature net only, no scatter) is timed separately, with the bytes it has to move
(voxels + num_points + coors in, [M, C] out, computed from the shapes) over that time.

    python tools/bench_pillar_encoder.py [--iters 20] [--warmup 5] [--rounds 5] [--json out.json]
"""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bevfusion_amd import pillar_encoder as pe  # noqa: E402

_spec = importlib.util.spec_from_file_location("cases", os.path.join(ROOT, "tests", "golden", "make_pillar_encoder_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def torch_reference(net, scatter, feats, num, coors, B):
    """(i): the reference's forward, op for op, on GPU tensors."""
    f = feats.clone() if net.mode == pe.MODE_RADAR else feats
    x = net._decorate_host(f, num, coors)
    for layer in net.layers:
        x = layer(x)
    x = x.squeeze(1)
    canvases = []
    for b in range(B):
        canvas = torch.zeros(scatter.in_channels, scatter.nx * scatter.ny, dtype=x.dtype, device=x.device)
        mask = coors[:, 0] == b
        this = coors[mask, :]
        idx = (this[:, 1] * scatter.ny + this[:, 2]).type(torch.long)
        canvas[:, idx] = x[mask, :].t()
        canvases.append(canvas)
    return torch.stack(canvases, 0).view(B, scatter.in_channels, scatter.nx, scatter.ny)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pillar_encoder needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    results = {}
    for case, M, shape in (("radar", 60000, (128, 128)), ("pillar", 30000, (512, 512))):
        c = gen.CASES[case]
        cls = pe.PillarFeatureNet if c["kind"] == "pillar" else pe.RadarFeatureNet
        net = cls(**gen.net_kwargs(case))
        st = gen.state([(k, tuple(v.shape)) for k, v in net.state_dict().items()], c["seed"])
        net.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
        net = net.to(dev).eval()
        scatter = pe.PointPillarsScatter(64, shape)
        B = 4 if case == "radar" else 2          # 2 x 128 x 128 cells cannot hold 60 000 distinct radar pillars: four samples
        feats, num, coors = (torch.from_numpy(a).to(dev) for a in gen.inputs(case, M=M, seed=31, B=B))

        def run(fused):
            net.use_fused = fused
            return scatter(net(feats, num, coors), coors, B)

        paths = {"torch_reference": lambda: torch_reference(net, scatter, feats, num, coors, B),
                 "unfused": lambda: run(False), "fused": lambda: run(True),
                 "fused_net_only": lambda: net._fused(feats, num, coors)}
        with torch.no_grad():
            ref = paths["torch_reference"]()
            for k in ("unfused", "fused"):
                got = paths[k]()
                err = float((got - ref).abs().max()) / float(ref.abs().max())
                assert err < 1e-5, (case, k, err)          # the three paths compute the same pseudo image
            for fn in paths.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            rounds = {k: [] for k in paths}
            for _ in range(args.rounds):
                for k, fn in paths.items():
                    rounds[k].append(timed(fn, args.iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
        P, F = feats.shape[1:]
        nbytes = M * P * F * 4 + M * 4 + M * 16 + M * 64 * 4
        results[case] = dict(pillars=M, ms=med, spread={k: [min(v), max(v)] for k, v in rounds.items()}, fused_kernel_bytes=nbytes,
                             fused_kernel_GBps=nbytes / (med["fused_net_only"] * 1e-3) / 1e9)
    line = json.dumps(results)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
