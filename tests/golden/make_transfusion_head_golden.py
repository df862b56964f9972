"""Writes tests/golden/transfusion_head_ref.npz: recorded outputs of the REFERENCE's FFN and TransFusionHead.forward_single.

The reference's `mmdet3d/models/utils/transformer.py` and `mmdet3d/models/heads/bbox/transfusion.py` are read and exec'd at run
time on CPU torch with one thread.  Their `mmcv`, `mmdet` and `mmdet3d.core` imports are stubbed: this file carries its own
conv -> norm -> ReLU `ConvModule` stand-in (children `conv`, `bn`, `activate`, as mmcv names them) and a `build_conv_layer` over
torch's classes; `HEADS.register_module` is the identity, `multi_apply` maps, the loss / coder / assigner builders return None.
Nothing of the reference's text is stored: only the SHA-256 of the seeded inputs and weights and the recorded results.  Inputs and
weights are NOT stored: `ffn_inputs` / `head_inputs` / `weights` regenerate them with numpy alone (the tests import this file for
them and check the stored digest).  BatchNorm running statistics are non-trivial.

Two kinds of recording:

  * `ffn`: FFN(128, the YAML's six heads (2, 1, 3, 2, 2, 10), head_conv 64) on x [2, 128, 17] in eval mode: the float64 output of
    a `.double()` copy and the reference's own fp32 output, per head;
  * `single` / `aux`: forward_single of a head with in_channels 32, hidden 128, 10 classes, a 12 x 12 BEV, 24 proposals,
    nms_kernel_size 3, nuScenes, eval mode; `single` has one decoder layer, `aux` two with auxiliary=True.  Stored: the state-dict
    names and shapes, the proposal classes and indices, the fp32 output dict and the float64 output dict of a `.double()` copy.

`yaml.head_cfg` is `model.heads.object` of the reference's `configs/nuscenes/det/transfusion/secfpn/lidar/voxelnet_0p075.yaml` chain
as JSON (settings only), so that the tests build the full-size head where the reference's configs are not at hand.

The weight seed of a forward recording is searched until two conditions on the REFERENCE's suppressed heatmap hold: at least
num_proposals + 1 suppressed scores are non-zero, and the top num_proposals + 1 scores are pairwise at least 1e-4 apart.  Together
they make the selection independent of the convolution's summation order and of the reference's unstable argsort.  Both are
asserted and the smallest gap is stored.

    python tests/golden/make_transfusion_head_golden.py
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
OUT = os.path.join(HERE, "transfusion_head_ref.npz")
REF = "/root/reference/mmdet3d"

FFN_B, FFN_IN, FFN_HEAD_CONV, FFN_P = 2, 128, 64, 17
FFN_HEADS = dict(center=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2), heatmap=(10, 2))
FFN_SEED = 2203

B, IN_CHANNELS, HIDDEN, CLASSES, BEV, PROPOSALS = 2, 32, 128, 10, 12, 24
MIN_GAP = 1e-4
YAML_LEAF = "nuscenes/det/transfusion/secfpn/lidar/voxelnet_0p075.yaml"
CASES = {"single": dict(layers=1, input_seed=811), "aux": dict(layers=2, input_seed=812)}


def head_kwargs(tag):
    """Constructor arguments of the recorded head (losses, coder and train_cfg left out: forward does not read them)."""
    return dict(num_proposals=PROPOSALS, auxiliary=True, in_channels=IN_CHANNELS, hidden_channel=HIDDEN, num_classes=CLASSES,
                num_decoder_layers=CASES[tag]["layers"], num_heads=8, nms_kernel_size=3, ffn_channel=256, dropout=0.1, bn_momentum=0.1,
                activation="relu", common_heads=dict(center=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2)),
                loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0),
                loss_heatmap=dict(type="GaussianFocalLoss", reduction="mean", loss_weight=1.0),
                loss_bbox=dict(type="L1Loss", reduction="mean", loss_weight=0.25),
                test_cfg=dict(dataset="nuScenes", grid_size=[BEV * 8, BEV * 8, 1], out_size_factor=8, voxel_size=[0.075, 0.075],
                              pc_range=[-54.0, -54.0], nms_type=None))


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
        elif name.endswith(".weight"):                                # BatchNorm / LayerNorm scale
            value = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        else:                                                         # biases, BatchNorm / LayerNorm shift
            value = rng.uniform(-0.2, 0.2, shape).astype(np.float32)
        out[name] = value
    return out


@functools.lru_cache(maxsize=None)
def ffn_inputs():
    """x [B, Cin, P] fp32."""
    return np.random.default_rng(FFN_SEED).standard_normal((FFN_B, FFN_IN, FFN_P)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def head_inputs(tag):
    """BEV features [B, in_channels, H, W] fp32."""
    return np.random.default_rng(CASES[tag]["input_seed"]).standard_normal((B, IN_CHANNELS, BEV, BEV)).astype(np.float32)


def digest(inputs, w):
    return sha(inputs, *[w[name] for name in w])


# ---- the stubs -------------------------------------------------------------------------------------------------------------------
def _stubs():
    import torch
    from torch import nn

    convs = {"Conv1d": nn.Conv1d, "Conv2d": nn.Conv2d}
    norms = {"BN1d": nn.BatchNorm1d, "BN2d": nn.BatchNorm2d}

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

    class _Heads:
        @staticmethod
        def register_module(*args, **kwargs):
            return lambda cls: cls

    def multi_apply(func, *args, **kwargs):
        results = map(functools.partial(func, **kwargs) if kwargs else func, *args)
        return tuple(map(list, zip(*results)))

    nothing = lambda *a, **k: None   # noqa: E731
    return dict(torch=torch, ConvModule=ConvModule, build_conv_layer=build_conv_layer, HEADS=_Heads, multi_apply=multi_apply,
                nothing=nothing)


def load_reference():
    """(namespace of transformer.py, namespace of transfusion.py), exec'd with the stubs in place."""
    s = _stubs()
    s["torch"].set_num_threads(1)
    nothing = s["nothing"]
    names = ["mmcv", "mmcv.cnn", "mmcv.runner", "mmdet", "mmdet.core", "mmdet3d", "mmdet3d.core", "mmdet3d.models", "mmdet3d.models.builder",
             "mmdet3d.models.utils", "mmdet3d.ops", "mmdet3d.ops.iou3d", "mmdet3d.ops.iou3d.iou3d_utils"]
    saved = {name: sys.modules.get(name) for name in names}
    mods = {name: types.ModuleType(name) for name in names}
    mods["mmcv.cnn"].__dict__.update(ConvModule=s["ConvModule"], build_conv_layer=s["build_conv_layer"], kaiming_init=nothing)
    mods["mmcv.runner"].__dict__.update(force_fp32=lambda *a, **k: (lambda f: f))
    mods["mmdet3d.core"].__dict__.update(PseudoSampler=nothing, circle_nms=nothing, draw_heatmap_gaussian=nothing, gaussian_radius=nothing,
                                         xywhr2xyxyr=nothing)
    mods["mmdet3d.models.builder"].__dict__.update(HEADS=s["HEADS"], build_loss=nothing)
    mods["mmdet3d.ops.iou3d.iou3d_utils"].__dict__.update(nms_gpu=nothing)
    mods["mmdet.core"].__dict__.update(AssignResult=nothing, build_assigner=nothing, build_bbox_coder=nothing, build_sampler=nothing,
                                       multi_apply=s["multi_apply"])
    sys.modules.update(mods)
    try:
        path = os.path.join(REF, "models/utils/transformer.py")
        tns = {"__name__": "reference_transformer"}
        exec(compile(open(path).read(), path, "exec"), tns)
        mods["mmdet3d.models.utils"].__dict__.update(FFN=tns["FFN"], PositionEmbeddingLearned=tns["PositionEmbeddingLearned"],
                                                     TransformerDecoderLayer=tns["TransformerDecoderLayer"])
        path = os.path.join(REF, "models/heads/bbox/transfusion.py")
        hns = {"__name__": "reference_transfusion"}
        exec(compile(open(path).read(), path, "exec"), hns)
    finally:
        for name, module in saved.items():
            if module is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = module
    return tns, hns


def _load(module, w):
    import torch

    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)


def record_ffn(tns, out):
    import torch

    ffn = tns["FFN"](FFN_IN, dict(FFN_HEADS), head_conv=FFN_HEAD_CONV)
    state = ffn.state_dict()
    shapes = [(k, tuple(v.shape)) for k, v in state.items()]
    w = weights(shapes, FFN_SEED)
    _load(ffn, w)
    ffn.eval()
    x = torch.from_numpy(ffn_inputs())
    with torch.no_grad():
        out32 = ffn(x)
        out64 = copy.deepcopy(ffn).double()(x.double())
    out["ffn.names"] = np.array([k for k, _ in shapes])
    out["ffn.shapes"] = np.array([",".join(str(d) for d in s) for _, s in shapes])
    out["ffn.heads"] = np.array(list(FFN_HEADS))
    out["ffn.inputs_sha256"] = np.array(digest(ffn_inputs(), w))
    for name in FFN_HEADS:
        out[f"ffn.out64.{name}"] = out64[name].numpy()
        out[f"ffn.out32.{name}"] = out32[name].numpy()
        err = float((out32[name].double() - out64[name]).abs().max() / out64[name].abs().max())
        print(f"  ffn.{name}: |out| max {float(out64[name].abs().max()):.3f}, fp32 against float64 {err:.3e} of it")


def suppressed_scores(dense_heatmap, kernel=3, exempt=(8, 9)):
    """The suppressed sigmoid map [B, C * H * W] of transfusion.py:239-267 from the reference's dense_heatmap (a torch tensor)."""
    import torch
    import torch.nn.functional as F

    heat = dense_heatmap.detach().sigmoid()
    pad = kernel // 2
    local_max = torch.zeros_like(heat)
    local_max[:, :, pad:-pad, pad:-pad] = F.max_pool2d(heat, kernel_size=kernel, stride=1, padding=0)
    for c in exempt:
        local_max[:, c] = heat[:, c]
    return (heat * (heat == local_max)).reshape(heat.shape[0], -1)


def _run_head(hns, tag, seed):
    """-> (head, shapes, weights, fp32 dict, classes, indices, smallest gap of the top K + 1, non-zero scores) for one seed."""
    import torch

    head = hns["TransFusionHead"](**head_kwargs(tag))
    shapes = [(k, tuple(v.shape)) for k, v in head.state_dict().items()]
    w = weights(shapes, seed)
    _load(head, w)
    head.eval()
    with torch.no_grad():
        res = head.forward_single(torch.from_numpy(head_inputs(tag)), None, None)[0]
    flat = suppressed_scores(res["dense_heatmap"])
    order = flat.argsort(dim=-1, descending=True, stable=True)[:, :PROPOSALS + 1]
    top = flat.gather(1, order)
    gap = float((top[:, :-1] - top[:, 1:]).min())
    nonzero = int((flat > 0).sum(1).min())
    cells = BEV * BEV
    return head, shapes, w, res, order[:, :PROPOSALS] // cells, order[:, :PROPOSALS] % cells, gap, nonzero


def record_head(hns, tag, out):
    import torch
    from torch import nn

    for seed in range(1, 400):
        head, shapes, w, res32, cls, idx, gap, nonzero = _run_head(hns, tag, seed)
        if nonzero >= PROPOSALS + 1 and gap >= MIN_GAP:
            break
    else:
        raise RuntimeError(f"{tag}: no seed separates the top {PROPOSALS + 1} scores by {MIN_GAP}")
    assert nonzero >= PROPOSALS + 1 and gap >= MIN_GAP
    # the reference's own (unstable) argsort chose the same proposals: the scores are distinct
    assert torch.equal(head.query_labels, cls), "the reference's selection differs from the stable one"
    flat = suppressed_scores(res32["dense_heatmap"]).view(B, CLASSES, -1)
    assert torch.equal(res32["query_heatmap_score"], flat.gather(2, idx[:, None, :].expand(-1, CLASSES, -1)))

    class ToDouble(nn.Module):
        def forward(self, x):
            return x.double()

    head64 = copy.deepcopy(head).double()
    head64.bev_pos = head64.bev_pos.double()                           # a plain attribute: .double() leaves it in fp32
    head64.class_encoding = nn.Sequential(ToDouble(), head64.class_encoding)   # the reference feeds it one_hot.float()
    with torch.no_grad():
        res64 = head64.forward_single(torch.from_numpy(head_inputs(tag)).double(), None, None)[0]
    assert torch.equal(head64.query_labels, cls), "the float64 copy selects other proposals"

    out[f"{tag}.seed"] = np.array(seed)
    out[f"{tag}.names"] = np.array([k for k, _ in shapes])
    out[f"{tag}.shapes"] = np.array([",".join(str(d) for d in s) for _, s in shapes])
    out[f"{tag}.inputs_sha256"] = np.array(digest(head_inputs(tag), w))
    out[f"{tag}.proposal_class"] = cls.numpy()
    out[f"{tag}.proposal_index"] = idx.numpy()
    out[f"{tag}.min_gap"] = np.array(gap)
    out[f"{tag}.keys"] = np.array(list(res32))
    print(f"  {tag}: seed {seed}, {len(shapes)} state entries, {nonzero} non-zero scores, smallest gap {gap:.3e}")
    for key in res32:
        out[f"{tag}.out32.{key}"] = res32[key].numpy()
        out[f"{tag}.out64.{key}"] = res64[key].numpy()
        err = float((res32[key].double() - res64[key]).abs().max() / res64[key].abs().max())
        print(f"    {key} {tuple(res32[key].shape)}: |out| max {float(res64[key].abs().max()):.3f}, fp32 against float64 {err:.3e} of it")


def yaml_head_config():
    """`model.heads.object` of the reference's configs/nuscenes/det/transfusion chain (settings only), through the project's loader."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from bevfusion_amd.config import load_config

    cfg = load_config(os.path.join(os.path.dirname(REF), "configs", YAML_LEAF))
    return cfg["model"]["heads"]["object"]


def main():
    tns, hns = load_reference()
    out = {"yaml.leaf": np.array(YAML_LEAF), "yaml.head_cfg": np.array(json.dumps(yaml_head_config()))}
    record_ffn(tns, out)
    for tag in CASES:
        record_head(hns, tag, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
