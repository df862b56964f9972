"""Times the TransFusion decoder's cross-attention on an MI355X at the configuration's shape (8 heads of 16, 200 queries, 32 400 BEV
keys, B = 1, 4, 8), three ways on the same device and the same random (not zero) tensors:

  (i)   the reference's formulation, the yardstick (mmdet3d/models/utils/transformer.py:314-315, 405, 428-491): its two `torch.equal`
        lines on a cross-attention's arguments (query and key differ in shape, so the first line is decided without a compare; key
        and value are distinct, equal tensors as in the layer, so the second compares S x B x 128 floats and syncs), q scaled,
        `bmm`, `softmax`, `dropout` (eval: identity), `bmm`, and the head-averaged weights nobody reads: the [heads, L, S] fp32
        logits are written and read again;
  (ii)  `F.scaled_dot_product_attention` on the same tensors, if it takes head dimension 16: reported only;
  (iii) `decoder.fused_attention` forward, and forward + backward (fp32).

Host wall clock around one call ended by a device synchronise, after `--warmup` calls; the median of `--iters` calls and the spread
(median absolute deviation) of each.  The tool FAILS if (iii) forward is not faster than (i) by more than the two spreads together
at every B: (i) cannot avoid about 0.8 GB of logits traffic per sample, the kernel's compulsory traffic is 33 MB.

    python tools/bench_decoder_attention.py [--iters 30] [--warmup 5] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bevfusion_amd import decoder  # noqa: E402

H, L, S, D = 8, 200, 32400, 16


def reference_formulation(query, key, value, q, k, v):
    """(i) on projected [B, L, E] / [B, S, E] tensors; query / key / value stand for the unprojected inputs the reference compares
    (transformer.py:314-315 as written)."""
    qkv_same = torch.equal(query, key) and torch.equal(key, value)
    kv_same = torch.equal(key, value)
    assert kv_same and not qkv_same
    B = q.shape[0]
    qh = (q * 0.25).reshape(B, L, H, D).permute(0, 2, 1, 3).reshape(B * H, L, D)
    kh = k.reshape(B, S, H, D).permute(0, 2, 1, 3).reshape(B * H, S, D)
    vh = v.reshape(B, S, H, D).permute(0, 2, 1, 3).reshape(B * H, S, D)
    w = F.dropout(F.softmax(torch.bmm(qh, kh.transpose(1, 2)), dim=-1), p=0.1, training=False)
    out = torch.bmm(w, vh).reshape(B, H, L, D).permute(0, 2, 1, 3).reshape(B, L, H * D)
    return out, w.view(B, H, L, S).sum(dim=1) / H


def sdpa(q, k, v):
    B = q.shape[0]
    split = lambda t: t.reshape(B, -1, H, D).transpose(1, 2)
    return F.scaled_dot_product_attention(split(q), split(k), split(v)).transpose(1, 2).reshape(B, L, H * D)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    times = np.array(times)
    med = float(np.median(times))
    return dict(median_us=med, spread_us=float(np.median(np.abs(times - med))), min_us=float(times.min()), iters=iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.iters >= 20
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), shape=dict(H=H, L=L, S=S, D=D), batches={})
    ok = True
    for B in args.batches:
        gen = torch.Generator(device=dev).manual_seed(100 + B)
        q = torch.randn(B, L, H * D, device=dev, generator=gen)
        k = torch.randn(B, S, H * D, device=dev, generator=gen)
        v = torch.randn(B, S, H * D, device=dev, generator=gen)
        query, key = torch.randn(L, B, H * D, device=dev, generator=gen), torch.randn(S, B, H * D, device=dev, generator=gen)
        value = key.clone()                                                    # the layer builds key and value as two equal tensors
        row = dict(plan=decoder.attention_plan(B, H, L, S))
        with torch.no_grad():
            ref_out = reference_formulation(query, key, value, q, k, v)[0]
            row["max_abs_diff_to_reference"] = float((decoder.fused_attention(q, k, v) - ref_out).abs().max())
            row["reference"] = timed(lambda: reference_formulation(query, key, value, q, k, v), args.iters, args.warmup)
            try:
                row["sdpa_max_abs_diff"] = float((sdpa(q, k, v) - ref_out).abs().max())
                row["sdpa"] = timed(lambda: sdpa(q, k, v), args.iters, args.warmup)
            except RuntimeError as e:                                              # head dimension 16 not taken
                row["sdpa"] = dict(error=str(e).split("\n")[0])
            row["fused_forward"] = timed(lambda: decoder.fused_attention(q, k, v), args.iters, args.warmup)
        qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
        dout = torch.randn(B, L, H * D, device=dev, generator=gen)

        def step():
            qg.grad = kg.grad = vg.grad = None
            decoder.fused_attention(qg, kg, vg).backward(dout)

        row["fused_forward_backward"] = timed(step, args.iters, args.warmup)
        ref, fwd = row["reference"], row["fused_forward"]
        row["speedup_over_reference"] = ref["median_us"] / fwd["median_us"]
        if "median_us" in row["sdpa"]:
            row["fused_over_sdpa"] = fwd["median_us"] / row["sdpa"]["median_us"]
        row["faster_than_reference"] = fwd["median_us"] + fwd["spread_us"] + ref["spread_us"] < ref["median_us"]
        ok = ok and row["faster_than_reference"]
        result["batches"][str(B)] = row
        print(f"B {B}: reference {ref['median_us']:.0f} +- {ref['spread_us']:.0f} us | sdpa "
              f"{row['sdpa'].get('median_us', float('nan')):.0f} us | fused forward {fwd['median_us']:.0f} +- {fwd['spread_us']:.0f} us "
              f"({row['speedup_over_reference']:.1f} x the reference) | forward + backward "
              f"{row['fused_forward_backward']['median_us']:.0f} us", flush=True)
    result["ok"] = ok
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps(dict(ok=ok)))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
