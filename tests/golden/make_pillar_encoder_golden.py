"""Writes tests/golden/pillar_encoder_ref.npz: recorded outputs of the REFERENCE's PillarFeatureNet / RadarFeatureNet /
PointPillarsScatter on seeded inputs.

The reference's `pillar_encoder.py` and `radar_encoder.py` are exec'd unmodified from where they lie, under inert `sys.modules`
stubs for the imports that cannot be satisfied here (mmcv, mmdet, mmdet3d, torchvision.utils, flash_attn), on CPU torch with one
thread.  No reference source is copied; only inputs' digests and recorded results go into the file.  Inputs and weights are NOT
stored: `inputs()`, `state()`, `loss_weights()` and `scatter_inputs()` below regenerate them from the seed (the tests import
this file for them and check the stored SHA-256).

Sizes: the pillar cases hold 800 and 200 pillars and the radar case 360, so that everything recorded (three [M, 64] outputs per
case, the f_cluster columns, every weight gradient of the 47 -> 128 -> 128 -> 128 -> 64 radar net) fits one file below 1 MiB.
The float64 recomputation is stored as its fp32 rounding plus the int8-quantised remainder (relative error below 1e-9, three
orders below the fp32 error it measures).

    python tests/golden/make_pillar_encoder_golden.py
"""
import hashlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pillar_encoder_ref.npz")
REF_DIR = "/root/reference/mmdet3d/models/backbones"

RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
NORM = dict(type="BN1d", eps=1e-3, momentum=0.01)
CASES = {
    "pillar": dict(kind="pillar", in_channels=5, feat_channels=[64, 64], with_distance=False, voxel_size=[0.2, 0.2, 8], P=20,
                   M=800, B=2, seed=101),
    "pillar_dist": dict(kind="pillar", in_channels=5, feat_channels=[64], with_distance=True, voxel_size=[0.2, 0.2, 8], P=20,
                        M=200, B=2, seed=102),
    "radar": dict(kind="radar", in_channels=45, feat_channels=[128, 128, 128, 64], with_distance=False,
                  voxel_size=[0.8, 0.8, 8], P=20, M=360, B=2, seed=103),
}
SCATTER_CASES = {
    "scatter512": dict(nx=512, ny=512, C=64, B=2, M=3000, dup=0, stray=0, seed=201),
    "scatter128": dict(nx=128, ny=128, C=64, B=2, M=500, dup=0, stray=0, seed=202),
    "scatter128_dup": dict(nx=128, ny=128, C=64, B=2, M=500, dup=60, stray=25, seed=203),
}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def net_kwargs(case):
    c = CASES[case]
    return dict(in_channels=c["in_channels"], feat_channels=list(c["feat_channels"]), with_distance=c["with_distance"],
                voxel_size=list(c["voxel_size"]), point_cloud_range=list(RANGE), norm_cfg=dict(NORM))


def grid(case):
    vx, vy = CASES[case]["voxel_size"][:2]
    return int(round((RANGE[3] - RANGE[0]) / vx)), int(round((RANGE[4] - RANGE[1]) / vy))


def inputs(case, M=None, seed=None, P=None, B=None):
    """(features [M, P, F] fp32, num_points [M] int32, coors [M, 4] int32 (b, x, y, z)): distinct cells, num_points uniform in
    1..P, real rows uniform inside their own cell, padded rows zero."""
    c = CASES[case]
    M, P, B = M or c["M"], P or c["P"], B or c["B"]
    rng = np.random.default_rng(c["seed"] if seed is None else seed)
    nx, ny = grid(case)
    vx, vy = c["voxel_size"][:2]
    cells = rng.choice(B * nx * ny, size=M, replace=False)
    coors = np.zeros((M, 4), np.int32)
    coors[:, 0], coors[:, 1], coors[:, 2] = cells // (nx * ny), cells % (nx * ny) // ny, cells % ny
    num = rng.integers(1, P + 1, size=M).astype(np.int32)
    F = c["in_channels"]
    f = np.empty((M, P, F), np.float64)
    f[:, :, 0] = RANGE[0] + (coors[:, 1:2] + rng.random((M, P))) * vx
    f[:, :, 1] = RANGE[1] + (coors[:, 2:3] + rng.random((M, P))) * vy
    f[:, :, 2] = rng.uniform(RANGE[2], RANGE[5], (M, P))
    f[:, :, 3:] = rng.uniform(-1.0, 1.0, (M, P, F - 3))
    f *= (np.arange(P)[None, :] < num[:, None])[:, :, None]
    return f.astype(np.float32), num, coors


def inject_nonfinite(features):
    """A NaN, a +inf and a -inf in real rows of the first three pillars (row 0 is always real): the nan_to_num case."""
    f = features.copy()
    f[0, 0, 5], f[1, 0, 6], f[2, 0, 7] = np.nan, np.inf, -np.inf
    return f


def state(shapes, seed):
    """Seeded, non-trivial parameters and BatchNorm statistics for a state dict given as [(key, shape)] in order."""
    rng = np.random.default_rng(seed + 1000)
    out = {}
    for key, shape in shapes:
        if key.endswith("num_batches_tracked"):
            out[key] = np.asarray(3, np.int64)
        elif key.endswith("linear.weight"):
            out[key] = (rng.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
        elif key.endswith("norm.weight") or key.endswith("running_var"):
            out[key] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif key.endswith("norm.bias"):
            out[key] = (0.2 * rng.standard_normal(shape)).astype(np.float32)
        elif key.endswith("running_mean"):
            out[key] = (0.3 * rng.standard_normal(shape)).astype(np.float32)
        else:
            raise KeyError(key)
    return out


def loss_weights(case, shape):
    return np.random.default_rng(CASES[case]["seed"] + 2000).standard_normal(shape).astype(np.float32)


def scatter_inputs(name):
    """(feats [M, C] fp32, coors [M, 4] int32): distinct cells; `dup` rows then repeat the cell of an earlier row and `stray`
    rows carry a batch index outside [0, B)."""
    c = SCATTER_CASES[name]
    rng = np.random.default_rng(c["seed"])
    M, nx, ny, B = c["M"], c["nx"], c["ny"], c["B"]
    cells = rng.choice(B * nx * ny, size=M, replace=False)
    coors = np.zeros((M, 4), np.int32)
    coors[:, 0], coors[:, 1], coors[:, 2] = cells // (nx * ny), cells % (nx * ny) // ny, cells % ny
    if c["dup"]:
        dst = rng.choice(np.arange(M // 2, M), size=c["dup"], replace=False)
        coors[dst] = coors[rng.integers(0, M // 2, size=c["dup"])]
    if c["stray"]:
        rows = rng.choice(M, size=c["stray"], replace=False)
        coors[rows, 0] = np.where(rng.random(c["stray"]) < 0.5, -1, B)
    feats = rng.standard_normal((M, c["C"])).astype(np.float32)
    return feats, coors


def scatter_grad(name):
    c = SCATTER_CASES[name]
    return np.random.default_rng(c["seed"] + 2000).standard_normal((c["B"], c["C"], c["nx"], c["ny"]), dtype=np.float32)


def scatter_winners(name):
    """(cell ids b * nx * ny + x * ny + y, winning row) of the non-empty cells, ascending: the highest valid row of each cell."""
    c = SCATTER_CASES[name]
    _, coors = scatter_inputs(name)
    ok = (coors[:, 0] >= 0) & (coors[:, 0] < c["B"])
    cell = (coors[:, 0].astype(np.int64) * c["nx"] + coors[:, 1]) * c["ny"] + coors[:, 2]
    best = {}
    for row in np.nonzero(ok)[0]:
        best[int(cell[row])] = int(row)
    cells = np.array(sorted(best), np.int64)
    return cells, np.array([best[int(k)] for k in cells], np.int32)


def pack64(a):
    """float64 array -> (fp32 rounding, int8 remainder, remainder scale)."""
    hi = a.astype(np.float32)
    lo = a - hi.astype(np.float64)
    scale = max(float(np.max(np.abs(lo))), 1e-300) / 127.0
    return hi, np.round(lo / scale).astype(np.int8), np.float64(scale)


def unpack64(hi, q, scale):
    return hi.astype(np.float64) + q.astype(np.float64) * float(scale)


def rel_err(a, b):
    """max |a - b| / max |b| (b: the float64 value)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


# ---- the reference, exec'd under stubs -------------------------------------------------------------------------------------
def load_reference():
    import torch
    from torch import nn

    registry = {}

    class _Backbones:
        def register_module(self, *a, **k):
            def deco(cls):
                registry[cls.__name__] = cls
                return cls
            return deco

    def build_backbone(cfg):
        cfg = dict(cfg)
        return registry[cfg.pop("type")](**cfg)

    def build_norm_layer(cfg, num_features, postfix=""):
        cfg = dict(cfg)
        typ = cfg.pop("type")
        assert typ == "BN1d", typ
        cfg.pop("requires_grad", None)
        return "bn" + str(postfix), nn.BatchNorm1d(num_features, **cfg)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    stubs = {
        "mmcv": mod("mmcv"),
        "mmcv.cnn": mod("mmcv.cnn", build_norm_layer=build_norm_layer, build_conv_layer=None),
        "mmcv.cnn.resnet": mod("mmcv.cnn.resnet", make_res_layer=None, BasicBlock=None),
        "mmcv.cnn.bricks": mod("mmcv.cnn.bricks"),
        "mmcv.cnn.bricks.non_local": mod("mmcv.cnn.bricks.non_local", NonLocal2d=None),
        "mmdet": mod("mmdet"),
        "mmdet.models": mod("mmdet.models", BACKBONES=_Backbones()),
        "mmdet3d": mod("mmdet3d"),
        "mmdet3d.models": mod("mmdet3d.models"),
        "mmdet3d.models.builder": mod("mmdet3d.models.builder", build_backbone=build_backbone),
        "mmdet3d.ops": mod("mmdet3d.ops", feature_decorator=None),
        "torchvision": mod("torchvision"),
        "torchvision.utils": mod("torchvision.utils", save_image=None),
        "flash_attn": mod("flash_attn"),
        "flash_attn.flash_attention": mod("flash_attn.flash_attention", FlashMHA=None),
    }
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        mods = {}
        for fname in ("pillar_encoder.py", "radar_encoder.py"):
            path = os.path.join(REF_DIR, fname)
            m = types.ModuleType("reference_" + fname[:-3])
            exec(compile(open(path).read(), path, "exec"), m.__dict__)
            mods[fname[:-3]] = m
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    torch.set_num_threads(1)
    return mods["pillar_encoder"], mods["radar_encoder"]


def _layers(net):
    return net.pfn_layers if hasattr(net, "pfn_layers") else net.rfn_layers


def _run(net, feats, num, coors, wloss, train):
    """One forward (+ backward in train mode) of a reference net; returns numpy results."""
    import torch

    seen = {}
    hook = _layers(net)[0].register_forward_pre_hook(lambda m, a: seen.__setitem__("x", a[0].detach().clone()))
    net.train(train)
    net.zero_grad()
    with torch.set_grad_enabled(train):
        out = net(feats.clone(), num, coors)
        if train:
            (out * wloss.to(out.dtype)).sum().backward()
    hook.remove()
    res = dict(out=out.detach().numpy(), decor=seen["x"].numpy())
    if train:
        res["grads"] = {k: p.grad.detach().numpy().copy() for k, p in net.named_parameters()}
        res["stats"] = {k: v.detach().numpy().copy() for k, v in net.state_dict().items() if "running" in k or "tracked" in k}
    return res


def record_net(case, ref_pillar, ref_radar, out):
    import torch

    c = CASES[case]
    cls = ref_pillar.PillarFeatureNet if c["kind"] == "pillar" else ref_radar.RadarFeatureNet
    f, n, co = inputs(case)
    feats, num, coors = torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(co)

    def make(dtype):
        net = cls(**net_kwargs(case))
        shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict({k: torch.from_numpy(v) for k, v in state(shapes, c["seed"]).items()})
        return net.to(dtype), shapes

    net32, shapes = make(torch.float32)
    net64, _ = make(torch.float64)
    wloss = torch.from_numpy(loss_weights(case, (c["M"], c["feat_channels"][-1])))
    p = case + "."
    out[p + "state_keys"] = np.array(json.dumps([k for k, _ in shapes]))
    out[p + "inputs_sha256"] = np.array(sha(f, n, co))
    out[p + "state_sha256"] = np.array(sha(*state(shapes, c["seed"]).values()))

    e32 = _run(net32, feats, num, coors, wloss, False)
    e64 = _run(net64, feats.double(), num, coors, wloss, False)
    F = c["in_channels"]
    decor = e32["decor"].copy()
    if c["kind"] == "pillar":
        out[p + "fcluster"] = decor[:, :, F:F + 3][np.arange(c["P"])[None, :] < n[:, None]]   # real rows only, [sum(num), 3]
        decor[:, :, F:F + 3] = 0
    out[p + "decor_sha256"] = np.array(sha(decor))          # the decorated tensor with the f_cluster columns zeroed
    out[p + "eval_sha256"] = np.array(sha(e32["out"]))
    out[p + "eval64_hi"], out[p + "eval64_q"], out[p + "eval64_scale"] = pack64(e64["out"])
    out[p + "e_ref"] = np.float64(rel_err(e32["out"], e64["out"]))

    t32 = _run(net32, feats, num, coors, wloss, True)
    t64 = _run(net64, feats.double(), num, coors, wloss, True)
    out[p + "train_out"] = t32["out"]
    out[p + "train_out_err"] = np.float64(rel_err(t32["out"], t64["out"]))
    for k, v in t32["stats"].items():
        out[p + "train_stat." + k] = v
        if "tracked" not in k:
            out[p + "train_stat_err." + k] = np.float64(rel_err(v, t64["stats"][k]))
    for k, v in t32["grads"].items():
        out[p + "train_grad." + k] = v
        out[p + "train_grad_err." + k] = np.float64(rel_err(v, t64["grads"][k]))

    if c["kind"] == "radar":   # nan_to_num: decorate only (FLT_MAX rows overflow the layers by design)
        bad = _run(net32, torch.from_numpy(inject_nonfinite(f)), num, coors, wloss, False)
        assert not np.isnan(bad["decor"]).any() and np.abs(bad["decor"]).max() > 1e38
        out[p + "decor_nonfinite_sha256"] = np.array(sha(bad["decor"]))


def record_scatter(name, ref_pillar, out):
    import torch

    c = SCATTER_CASES[name]
    f, co = scatter_inputs(name)
    feats = torch.from_numpy(f).requires_grad_(True)
    mod = ref_pillar.PointPillarsScatter(in_channels=c["C"], output_shape=(c["nx"], c["ny"]))
    canvas = mod(feats, torch.from_numpy(co), c["B"])
    canvas.backward(torch.from_numpy(scatter_grad(name)))
    cells, rows = scatter_winners(name)
    flat = canvas.detach().numpy().reshape(c["B"], c["C"], -1)
    rebuilt = np.zeros_like(flat)
    rebuilt[cells // (c["nx"] * c["ny"]), :, cells % (c["nx"] * c["ny"])] = f[rows]
    assert np.array_equal(rebuilt, flat), "the reference's canvas is not 'highest row wins'"
    grad = feats.grad.numpy().copy()
    losers = np.setdiff1d(np.arange(c["M"]), rows)
    grad[losers] = 0          # the reference's index_put backward hands a loser its cell's gradient too
    p = name + "."
    out[p + "inputs_sha256"] = np.array(sha(f, co))
    out[p + "canvas_sha256"] = np.array(sha(flat))
    out[p + "cells"], out[p + "rows"] = cells, rows
    out[p + "grad_sha256"] = np.array(sha(grad))
    out[p + "nonzero_cells"] = np.int64(len(cells))


def main():
    ref_pillar, ref_radar = load_reference()
    out = {}
    for case in CASES:
        record_net(case, ref_pillar, ref_radar, out)
    for name in SCATTER_CASES:
        record_scatter(name, ref_pillar, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    for k in sorted(out):
        if k.endswith("e_ref") or "_err" in k:
            print(f"  {k} = {float(out[k]):.3e}")


if __name__ == "__main__":
    main()
