"""Times the camera Swin-T's eval-mode forward on an MI355X on 256 x 704 images in fp16, at 1 and 8 frames of six cameras:

  attention   the shifted attention of each of the four stages (64 x 176 x 96 / 3 heads, 32 x 88 x 192 / 6, 16 x 44 x 384 / 12,
              8 x 22 x 768 / 24) between the qkv Linear and the proj Linear, on ONE qkv tensor: "fused" is one launch of
              `bevamd_window_attention_forward`, "torch" mmdet's sequence (pad, roll, partition, q k^T, bias, mask, softmax, attn v,
              reverse, roll back, crop) written on the same qkv map.  The bytes the fused op must move (qkv once, out once) over the
              measured HBM rate of 6.29 TB/s are printed as its floor.
  nets        the whole Swin-T: "fused" (the module's default `fused_stages`), "fused_all" (every stage) and "torch"
              (`use_fused = False`) on the same module in the same session.

  ffn         the tail of a block of each stage the fused FFN serves, on ONE token tensor [B, H W, C]: "fused" is one
              launch of `bevamd_swin_ffn_forward`, "torch" the module's own `ffn(norm2(x), identity=x)`.  Moved bytes (x in, out out,
              the two weights once) over the HBM rate are printed as the fused op's floor.
  ffn_nets    the whole Swin-T under `use_fused = True`: "base" (`fused_ffn_stages = ()`), "ffn0" ((0,)) and "ffn01" ((0, 1)).

`--steps ffn ffn_nets --json profiles/swin_ffn_timing.json` writes the FFN measurement; without `--steps` the run is attention + nets.

Device events around `--iters` calls after `--warmup` calls, the paths alternating inside every round; the median round is reported
with the spread.

Every step runs in a child process of its own under `timeout`; a step that fails, faults or runs out of time ends the run and
nothing further is started on the GPU.

    python tools/bench_cam_swin.py [--steps attention nets] [--iters 20] [--warmup 3] [--rounds 5] [--frames 1 8]
                                   [--json profiles/cam_swin_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_bev_trunk import compare  # noqa: E402

IMAGE, CAMERAS = (256, 704), 6
HBM_BYTES_PER_S = 6.29e12
STEP_SECONDS = {"attention": 400, "nets": 400, "ffn": 300, "ffn_nets": 400}
DEFAULT_STEPS = ["attention", "nets"]
FFN_SETTINGS = {"base": (), "ffn0": (0,), "ffn01": (0, 1)}
STAGES = [((64, 176), 96, 3), ((32, 88), 192, 6), ((16, 44), 384, 12), ((8, 22), 768, 24)]
ALL_STAGES = (0, 1, 2, 3)


def randomise(module, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.copy_(torch.randn(p.shape, generator=g))
            elif p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * p[0].numel() ** -0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(0.8 + 0.4 * torch.rand(p.shape, generator=g))
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return module


def torch_attention(attn, qkv):
    """mmdet's ShiftWindowMSA + WindowMSA between the two Linear layers, on a qkv map [B, H, W, 3C] (a padded token's qkv is the
    Linear's bias)."""
    import torch

    w, ws, shift = attn.w_msa, attn.window_size, attn.shift_size
    B, H, W, C3 = qkv.shape
    C, heads, N = C3 // 3, w.num_heads, ws * ws
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    x = qkv
    if pad_r or pad_b:
        x = w.qkv.bias.expand(B, H + pad_b, W + pad_r, C3).clone()
        x[:, :H, :W] = qkv
    Hp, Wp = x.shape[1], x.shape[2]
    mask = None
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        img = torch.zeros((1, Hp, Wp, 1), device=qkv.device)
        cnt = 0
        for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for v in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[:, h, v, :] = cnt
                cnt += 1
        mw = attn.window_partition(img).view(-1, N)
        mask = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = mask.masked_fill(mask != 0, -100.0).masked_fill(mask == 0, 0.0).to(qkv.dtype)
    win = attn.window_partition(x).view(-1, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = win[0] * w.scale, win[1], win[2]
    a = q @ k.transpose(-2, -1)
    a = a + w.relative_position_bias_table[w.relative_position_index.view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous().unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        a = (a.view(-1, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    o = (torch.softmax(a, -1) @ v).transpose(1, 2).reshape(-1, ws, ws, C)
    o = attn.window_reverse(o, Hp, Wp)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o[:, :H, :W, :].contiguous() if pad_r or pad_b else o


def step_attention(args):
    import torch

    from bevfusion_amd import cam_swin as cs

    dev = torch.device("cuda:0")
    out = {}
    with torch.no_grad():
        for frames in args.frames:
            B = frames * CAMERAS
            for i, ((H, W), C, heads) in enumerate(STAGES):
                blk = randomise(cs.SwinBlock(C, heads, 4 * C, shift=True), 20 + i).to(dev).half().eval()
                attn = blk.attn
                qkv = torch.randn(B, H, W, 3 * C, generator=torch.Generator().manual_seed(i)).half().to(dev)
                bias = cs.fold_window_bias(attn.w_msa)
                paths = {"torch": lambda attn=attn, qkv=qkv: torch_attention(attn, qkv),
                         "fused": lambda attn=attn, qkv=qkv, bias=bias: cs.window_attention(qkv, bias, attn.w_msa.scale, attn.shift_size,
                                                                                            attn.w_msa.qkv.bias)}
                ref = paths["torch"]().float()
                err = float((paths["fused"]().float() - ref).abs().max()) / float(ref.abs().max())
                assert err < 2e-2, err                  # both paths compute the same attention (fp16 storage)
                med, spread = compare(paths, args.iters, args.warmup, args.rounds)
                moved = 2 * B * H * W * 4 * C
                out[f"frames{frames}/stage{i + 1}"] = dict(ms=med, spread=spread, speedup=med["torch"] / med["fused"], max_rel_diff=err,
                                                           moved_bytes=moved, hbm_floor_ms=moved / HBM_BYTES_PER_S * 1e3)
                print(f"frames{frames}/stage{i + 1}: {json.dumps(out[f'frames{frames}/stage{i + 1}'])}", file=sys.stderr, flush=True)
    return out


def step_nets(args):
    import torch

    from bevfusion_amd import cam_swin as cs

    dev = torch.device("cuda:0")
    net = randomise(cs.SwinTransformer(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], out_indices=[1, 2, 3],
                                       drop_path_rate=0.2), 7).to(dev).half().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    default = tuple(net.fused_stages)
    out = {"default_fused_stages": list(default)}
    with torch.no_grad():
        for frames in args.frames:
            x = torch.randn((frames * CAMERAS, 3) + IMAGE, generator=torch.Generator().manual_seed(30 + frames)).half().to(dev)

            def path(use, stages, x=x):
                def fn():
                    net.use_fused, net.fused_stages = use, stages
                    return net(x)
                return fn
            paths = {"torch": path(False, default), "fused_all": path(True, ALL_STAGES), "fused": path(True, default)}
            net.use_fused, net.fused_stages = True, ALL_STAGES
            assert net.fusable(x)
            ref = paths["torch"]()[-1].float()
            errs = {k: float((fn()[-1].float() - ref).abs().max()) / float(ref.abs().max()) for k, fn in paths.items()}
            assert max(errs.values()) < 5e-2, errs
            med, spread = compare(paths, args.iters, args.warmup, args.rounds)
            net.use_fused, net.fused_stages = True, default
            out[f"frames{frames}"] = dict(ms=med, spread=spread, speedup={k: med["torch"] / v for k, v in med.items() if k != "torch"},
                                          max_rel_diff=errs)
            print(f"frames{frames}: {json.dumps(out[f'frames{frames}'])}", file=sys.stderr, flush=True)
    return out


def step_ffn(args):
    import torch

    from bevfusion_amd import cam_swin as cs

    dev = torch.device("cuda:0")
    out = {}
    with torch.no_grad():
        for frames in args.frames:
            B = frames * CAMERAS
            for i, ((H, W), C, heads) in enumerate(STAGES):
                blk = randomise(cs.SwinBlock(C, heads, 4 * C), 40 + i).to(dev).half().eval()
                if not cs.swin_ffn_spec(blk):
                    continue
                x = torch.randn(B, H * W, C, generator=torch.Generator().manual_seed(50 + i)).half().to(dev)
                paths = {"torch": lambda blk=blk, x=x: blk.ffn(blk.norm2(x), identity=x),
                         "fused": lambda blk=blk, x=x: cs.swin_ffn(x, blk.norm2, blk.ffn)}
                ref = paths["torch"]().float()
                err = float((paths["fused"]().float() - ref).abs().max()) / float(ref.abs().max())
                assert err < 2e-2, err                  # both paths compute the same tail (fp16 storage)
                med, spread = compare(paths, args.iters, args.warmup, args.rounds)
                T = B * H * W
                moved = 2 * T * C * 2 + 2 * 4 * C * C * 2
                torch_bytes = T * C * 2 * (2 + 5 + 8 + 5 + 3)          # LN 1 + 1, fc1 1 + 4, GELU 4 + 4, fc2 4 + 1, add 2 + 1 (in units of T C)
                key = f"frames{frames}/stage{i + 1}"
                out[key] = dict(ms=med, spread=spread, speedup=med["torch"] / med["fused"], max_rel_diff=err, tokens=T, channels=C,
                                moved_bytes=moved, hbm_floor_ms=moved / HBM_BYTES_PER_S * 1e3, torch_sequence_bytes=torch_bytes,
                                flop=4 * T * C * 4 * C)
                print(f"{key}: {json.dumps(out[key])}", file=sys.stderr, flush=True)
    return out


def step_ffn_nets(args):
    import torch

    from bevfusion_amd import cam_swin as cs

    dev = torch.device("cuda:0")
    net = randomise(cs.SwinTransformer(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], out_indices=[1, 2, 3],
                                       drop_path_rate=0.2), 7).to(dev).half().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    out = {"settings": {k: list(v) for k, v in FFN_SETTINGS.items()}, "default_fused_ffn_stages": list(net.fused_ffn_stages)}
    default = tuple(net.fused_ffn_stages)
    with torch.no_grad():
        for frames in args.frames:
            x = torch.randn((frames * CAMERAS, 3) + IMAGE, generator=torch.Generator().manual_seed(30 + frames)).half().to(dev)

            def path(stages, x=x):
                def fn():
                    net.use_fused, net.fused_ffn_stages = True, stages
                    return net(x)
                return fn
            paths = {k: path(v) for k, v in FFN_SETTINGS.items()}
            assert net.fusable(x)
            ref = paths["base"]()[-1].float()
            errs = {k: float((fn()[-1].float() - ref).abs().max()) / float(ref.abs().max()) for k, fn in paths.items()}
            assert max(errs.values()) < 5e-2, errs
            med, spread = compare(paths, args.iters, args.warmup, args.rounds)
            net.fused_ffn_stages = default
            out[f"frames{frames}"] = dict(ms=med, spread=spread, speedup={k: med["base"] / v for k, v in med.items() if k != "base"},
                                          max_rel_diff=errs)
            print(f"frames{frames}: {json.dumps(out[f'frames{frames}'])}", file=sys.stderr, flush=True)
    return out


STEPS = {"attention": step_attention, "nets": step_nets, "ffn": step_ffn, "ffn_nets": step_ffn_nets}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", nargs="+", choices=sorted(STEPS), default=DEFAULT_STEPS, help="the steps to run, each in a child process")
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_cam_swin needs a GPU: nothing is measured without one")
        print("RESULT " + json.dumps(STEPS[args.step](args)), flush=True)
        return
    results = {}
    for step in args.steps:
        seconds = STEP_SECONDS[step]
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(args.iters),
               "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--frames"] + [str(f) for f in args.frames]
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
