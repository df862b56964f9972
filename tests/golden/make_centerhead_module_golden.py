"""Writes tests/golden/centerhead_module_ref.npz: recorded outputs of the REFERENCE's SeparateHead and CenterHead.forward_single.

The reference's `mmdet3d/models/heads/bbox/centerpoint.py` is read and exec'd at run time on CPU torch with one thread.  Its `mmcv`,
`mmdet` and `mmdet3d` imports are stubbed: this file carries its own conv -> norm -> ReLU `ConvModule` stand-in (children `conv`,
`bn`, `activate`, as mmcv names them), a `build_conv_layer` over torch's classes, a `BaseModule` that is an `nn.Module`, and a
`build_head` that looks the type up in the exec'd namespace; `HEADS.register_module` is the identity, `multi_apply` maps, the loss
and coder builders return None.  Nothing of the reference's text is stored: only the SHA-256 of the seeded inputs and weights and
the recorded results.  Inputs and weights are NOT stored: `inputs` / `weights` regenerate them with numpy alone (the tests import
this file for them and check the stored digest).  BatchNorm running statistics are non-trivial, and the folded shift
(bias - running_mean * weight / sqrt(running_var + eps)) is positive on about half of the hidden channels, so that a hidden border
cell that is not zero shows in the output.

Three recordings, each with the state-dict names and shapes, the reference's own fp32 output and the float64 output of a
`.double()` copy, per head:

  * `sep3`: SeparateHead(64, {reg: (2, 2), height: (1, 2), dim: (3, 2), rot: (2, 2), vel: (2, 2), heatmap: (2, 2)}, final_kernel=3) on
    x [2, 64, 9, 11] in eval mode;
  * `sep1`: the same head with final_kernel=1;
  * `head`: CenterHead.forward_single with in_channels 32, share_conv_channel 64, tasks [["a"], ["b", "c"]], the YAML's common_heads,
    on a 12 x 12 map, in eval mode; keys `head.out64.<task>.<name>`.

`yaml.head_cfg` is `model.heads.object` of the reference's `configs/nuscenes/det/centerhead` chain as JSON (settings only), so that
the tests build the full-size head where the reference's configs are not at hand.

    python tests/golden/make_centerhead_module_golden.py
"""
import copy
import functools
import hashlib
import json
import os
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "centerhead_module_ref.npz")
REF = "/root/reference/mmdet3d"

SEP_HEADS = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2), heatmap=(2, 2))
SEP_SHAPE = (2, 64, 9, 11)
SEP = {"sep3": dict(final_kernel=3, seed=3301), "sep1": dict(final_kernel=1, seed=3302)}
HEAD_B, HEAD_IN, HEAD_MAP, HEAD_SEED = 2, 32, 12, 3303
HEAD_TASKS = [["a"], ["b", "c"]]
COMMON_HEADS = dict(reg=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2))
YAML_LEAF = "nuscenes/det/centerhead/lssfpn/camera/256x704/swint/default.yaml"


def head_kwargs():
    """Constructor arguments of the recorded head (losses, coder and the cfgs left out: forward does not read them)."""
    return dict(in_channels=HEAD_IN, tasks=[list(t) for t in HEAD_TASKS], common_heads=dict(COMMON_HEADS), share_conv_channel=64,
                separate_head=dict(type="SeparateHead", init_bias=-2.19, final_kernel=3))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def weights(shapes, seed):
    """name -> fp32 array (int64 for num_batches_tracked) for a list of (name, shape), from (name, seed) alone."""
    out = {}
    for name, shape in shapes:
        shape = tuple(int(s) for s in shape)
        rng = np.random.default_rng([zlib.crc32(name.encode()), int(seed)])
        if name.endswith("num_batches_tracked"):
            value = np.array(7, np.int64)
        elif len(shape) >= 2:                                         # xavier uniform over (fan_out, fan_in, receptive field)
            field = int(np.prod(shape[2:]))
            bound = np.sqrt(6.0 / ((shape[0] + shape[1]) * field))
            value = rng.uniform(-bound, bound, shape).astype(np.float32)
        elif name.endswith("running_mean"):
            value = rng.uniform(-0.5, 0.5, shape).astype(np.float32)
        elif name.endswith("running_var"):
            value = rng.uniform(0.5, 2.0, shape).astype(np.float32)
        elif name.endswith(".weight"):                                # BatchNorm scale
            value = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        else:                                                         # biases, BatchNorm shift
            value = rng.uniform(-0.2, 0.2, shape).astype(np.float32)
        out[name] = value
    return out


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """The recording's input, fp32: x [2, 64, 9, 11] of `sep3` / `sep1`, the BEV features [2, 32, 12, 12] of `head`."""
    if tag == "head":
        return np.random.default_rng(HEAD_SEED).standard_normal((HEAD_B, HEAD_IN, HEAD_MAP, HEAD_MAP)).astype(np.float32)
    return np.random.default_rng(SEP[tag]["seed"]).standard_normal(SEP_SHAPE).astype(np.float32)


def seed_of(tag):
    return HEAD_SEED if tag == "head" else SEP[tag]["seed"]


def digest(x, w):
    return sha(x, *[w[name] for name in w])


# ---- the stubs -------------------------------------------------------------------------------------------------------------------
def load_reference():
    """The namespace of centerpoint.py, exec'd with the stubs in place."""
    import torch
    from torch import nn

    torch.set_num_threads(1)
    convs = {"Conv2d": nn.Conv2d}
    norms = {"BN2d": nn.BatchNorm2d}
    ns = {"__name__": "reference_centerpoint"}

    def build_conv_layer(cfg, *args, **kwargs):
        cfg = dict(cfg or dict(type="Conv2d"))
        return convs[cfg.pop("type")](*args, **kwargs, **cfg)

    class ConvModule(nn.Module):
        """conv -> norm -> ReLU; bias="auto": no conv bias when a norm follows."""

        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias="auto", conv_cfg=None, norm_cfg=None):
            super().__init__()
            if bias == "auto":
                bias = norm_cfg is None
            self.conv = build_conv_layer(conv_cfg, in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias)
            self.bn = norms[norm_cfg["type"]](out_channels) if norm_cfg is not None else None
            self.activate = nn.ReLU(inplace=True)

        def forward(self, x):
            x = self.conv(x)
            if self.bn is not None:
                x = self.bn(x)
            return self.activate(x)

    class BaseModule(nn.Module):
        def __init__(self, init_cfg=None):
            super().__init__()
            self.init_cfg = init_cfg

    class _Heads:
        @staticmethod
        def register_module(*args, **kwargs):
            return lambda cls: cls

    def build_head(cfg):
        cfg = dict(cfg)
        return ns[cfg.pop("type")](**cfg)

    def multi_apply(func, *args, **kwargs):
        results = map(functools.partial(func, **kwargs) if kwargs else func, *args)
        return tuple(map(list, zip(*results)))

    nothing = lambda *a, **k: None   # noqa: E731
    names = ["mmcv", "mmcv.cnn", "mmcv.runner", "mmdet", "mmdet.core", "mmdet3d", "mmdet3d.core", "mmdet3d.models", "mmdet3d.models.builder",
             "mmdet3d.ops", "mmdet3d.ops.iou3d", "mmdet3d.ops.iou3d.iou3d_utils"]
    saved = {name: sys.modules.get(name) for name in names}
    mods = {name: types.ModuleType(name) for name in names}
    mods["mmcv.cnn"].__dict__.update(ConvModule=ConvModule, build_conv_layer=build_conv_layer)
    mods["mmcv.runner"].__dict__.update(BaseModule=BaseModule, force_fp32=lambda *a, **k: (lambda f: f))
    mods["mmdet3d.core"].__dict__.update(circle_nms=nothing, draw_heatmap_gaussian=nothing, gaussian_radius=nothing, xywhr2xyxyr=nothing)
    mods["mmdet3d.models.builder"].__dict__.update(HEADS=_Heads, build_loss=nothing, build_head=build_head)
    mods["mmdet3d.models"].__dict__.update(builder=mods["mmdet3d.models.builder"])
    mods["mmdet3d.ops.iou3d.iou3d_utils"].__dict__.update(nms_gpu=nothing)
    mods["mmdet.core"].__dict__.update(build_bbox_coder=nothing, multi_apply=multi_apply)
    sys.modules.update(mods)
    try:
        path = os.path.join(REF, "models/heads/bbox/centerpoint.py")
        exec(compile(open(path).read(), path, "exec"), ns)
    finally:
        for name, module in saved.items():
            if module is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = module
    return ns


def _load(module, w):
    import torch

    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)


def _record(tag, module, run, out):
    """Load the seeded state, run fp32 and a .double() copy, store names, shapes, digest and {key: array} of both."""
    import torch

    shapes = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    w = weights(shapes, seed_of(tag))
    _load(module, w)
    module.eval()
    x = torch.from_numpy(inputs(tag))
    with torch.no_grad():
        out32 = run(module, x)
        out64 = run(copy.deepcopy(module).double(), x.double())
    out[f"{tag}.names"] = np.array([k for k, _ in shapes])
    out[f"{tag}.shapes"] = np.array([",".join(str(d) for d in s) for _, s in shapes])
    out[f"{tag}.inputs_sha256"] = np.array(digest(inputs(tag), w))
    out[f"{tag}.keys"] = np.array(list(out32))
    positive = [float((w[k.replace("running_mean", "bias")] - w[k] * w[k.replace("running_mean", "weight")]
                       / np.sqrt(w[k.replace("running_mean", "running_var")] + 1e-5) > 0).mean())
                for k in w if k.endswith("bn.running_mean") and "shared_conv" not in k]
    assert 0.25 < min(positive) and max(positive) < 0.75, positive      # the border rule matters on every head
    print(f"  {tag}: {len(shapes)} state entries, folded shift positive on {min(positive):.2f} .. {max(positive):.2f} of the channels")
    for key in out32:
        out[f"{tag}.out32.{key}"] = out32[key].numpy()
        out[f"{tag}.out64.{key}"] = out64[key].numpy()
        err = float((out32[key].double() - out64[key]).abs().max() / out64[key].abs().max())
        print(f"    {key} {tuple(out32[key].shape)}: |out| max {float(out64[key].abs().max()):.3f}, fp32 against float64 {err:.3e} of it")


def yaml_head_config():
    """`model.heads.object` of the reference's configs/nuscenes/det/centerhead chain (settings only), through the project's loader."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from bevfusion_amd.config import load_config

    cfg = load_config(os.path.join(os.path.dirname(REF), "configs", YAML_LEAF))
    return cfg["model"]["heads"]["object"]


def main():
    ns = load_reference()
    out = {"yaml.leaf": np.array(YAML_LEAF), "yaml.head_cfg": np.array(json.dumps(yaml_head_config()))}
    for tag, spec in SEP.items():
        _record(tag, ns["SeparateHead"](64, dict(SEP_HEADS), final_kernel=spec["final_kernel"]), lambda m, x: m(x), out)

    def run_head(m, x):
        return {f"{t}.{name}": v for t, d in enumerate(m.forward_single(x)) for name, v in d.items()}

    _record("head", ns["CenterHead"](**head_kwargs()), run_head, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
