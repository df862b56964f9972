"""Writes tests/golden/head_losses_ref.npz: recorded outputs of the REFERENCE's head-loss statements on seeded inputs.

Read from where they lie and exec'd on CPU torch (one thread), once in fp32 and once in float64:
  * models/heads/bbox/transfusion.py:612-711: the statements of TransFusionHead.loss after get_targets, and 31-33, `clip_sigmoid`;
  * models/heads/bbox/centerpoint.py:597-633: the task loop of CenterHead.loss, 15-16, `clip_sigmoid`, and 368-388, `_gather_feat`;
each bound to a namespace object carrying the attributes they read.  mmdet is not installed: its three losses are RESTATED here
from mmdet 2.x (`gaussian_focal_loss`, `py_sigmoid_focal_loss`, `l1_loss`, `weight_reduce_loss` and the modules around them; on a
CPU tensor FocalLoss takes the `py_` path).  Nothing of the reference's text is stored: seeded inputs and recorded results only.

Per fixture: `in/*` the inputs, `loss/*` the float64 losses, `grad/*` the float64 autograd gradient of the SUM of all losses in
every prediction tensor, `err_loss/*` and `err_grad/*` the largest |fp32 run - float64 run| of each, and `num_pos/*`.  `cfg/*`: the
loss blocks of configs/nuscenes/det/{transfusion,centerhead}/default.yaml as JSON (settings).

Preconditions asserted here: every logit is at least 1e-2 away from +-log(9999) (no cell sits on the clamp edge); every target
that is not exactly 1 is at most 1 - 2^-20, EXCEPT the cells placed on purpose one fp32 step below 1 (asserted to be exactly
nextafter(1, 0): `t == 1` must be an equality, not a threshold).

    python tests/golden/make_head_losses_golden.py
"""
import json
import os
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "head_losses_ref.npz")
REF = "/root/reference"
CODE_WEIGHTS = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]
PIECES = (("center", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2))
CH_PIECES = (("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2))
BELOW_ONE = np.nextafter(np.float32(1), np.float32(0))

TF_CASES = {
    "tf_small": dict(B=2, C=3, S=11, L=3, K=17, D=10, seed=2001, ones=5, below=3, clamped=6),
    "tf_empty": dict(B=2, C=3, S=11, L=2, K=5, D=10, seed=2002, ones=0, below=0, clamped=2, empty=True),
    "tf_one_layer": dict(B=2, C=3, S=11, L=1, K=17, D=8, seed=2003, ones=4, below=1, clamped=2),
}
CH_CASES = {"ch_tasks": dict(B=2, classes=(1, 2, 2), S=13, M=9, seed=2004, live=((4, 3), (3, 2), (0, 0)))}


def _dense(rng, shape, ones, below, clamped):
    """-> (logits, target): seeded, with `clamped` logits at +-12, `ones` targets of exactly 1 and `below` one step under it."""
    n = int(np.prod(shape))
    x = (rng.standard_normal(n) * 2.0).astype(np.float32)
    t = (rng.random(n) ** 3 * 0.9).astype(np.float32)
    cells = rng.permutation(n)
    x[cells[:clamped]] = np.where(np.arange(clamped) % 2 == 0, 12.0, -12.0).astype(np.float32)
    t[cells[clamped:clamped + ones]] = 1.0
    t[cells[0]] = 1.0 if ones else t[cells[0]]                                   # one clamped cell is a positive
    t[cells[clamped + ones:clamped + ones + below]] = BELOW_ONE
    assert (np.abs(np.abs(x) - np.log(9999.0)) >= 1e-2).all()
    other = t[(t != 1) & (t != BELOW_ONE)]
    assert (other <= 1 - 2.0 ** -20).all() and ((t == BELOW_ONE).sum() == below)
    return x.reshape(shape), t.reshape(shape)


def tf_inputs(name):
    c = TF_CASES[name]
    rng = np.random.default_rng(c["seed"])
    B, C, S, L, K, D = c["B"], c["C"], c["S"], c["L"], c["K"], c["D"]
    P = L * K
    out = {}
    out["dense_heatmap"], out["heatmap_target"] = _dense(rng, (B, C, S, S), c["ones"], c["below"], c["clamped"])
    out["heatmap"] = (rng.standard_normal((B, C, P)) * 1.5).astype(np.float32)
    for n, w in PIECES[:5 if D == 10 else 4]:
        out[n] = rng.standard_normal((B, w, P)).astype(np.float32)
    labels = np.full((B, P), C, np.int64)
    if not c.get("empty"):
        pos = rng.random((B, P)) < 0.25
        labels[pos] = rng.integers(0, C, int(pos.sum()))
    out["labels"] = labels
    weights = np.ones((B, P), np.int64)
    weights[rng.random((B, P)) < 0.15] = 0                                      # zero-weight rows
    out["label_weights"] = weights
    out["bbox_targets"] = (rng.standard_normal((B, P, D)) * (labels < C)[..., None]).astype(np.float32)
    out["bbox_weights"] = np.repeat((labels < C)[..., None], D, 2).astype(np.float32)
    out["num_pos"] = np.int64((labels < C).sum())
    out["matched_ious"] = np.float32(0.0 if c.get("empty") else 0.37)
    assert (out["num_pos"] == 0) == bool(c.get("empty")) and (labels == C).any() and (weights == 0).any()
    return out


def ch_inputs(name):
    c = CH_CASES[name]
    rng = np.random.default_rng(c["seed"])
    B, S, M = c["B"], c["S"], c["M"]
    out = {}
    for t, ct in enumerate(c["classes"]):
        live = c["live"][t]
        ones = 3 if sum(live) else 0
        out[f"heatmap{t}"], out[f"heatmap_target{t}"] = _dense(rng, (B, ct, S, S), ones, 1, 2)
        for n, w in CH_PIECES:
            out[f"{n}{t}"] = rng.standard_normal((B, w, S, S)).astype(np.float32)
        ind = np.zeros((B, M), np.int64)
        mask = np.zeros((B, M), np.uint8)
        anno = np.zeros((B, M, 10), np.float32)
        for b in range(B):
            ind[b, :live[b]] = rng.permutation(S * S)[:live[b]]
            mask[b, :live[b]] = 1
            anno[b, :live[b]] = rng.standard_normal((live[b], 10))
        if t == 0:
            ind[0, 1] = ind[0, 0]                                               # two live slots on one cell
        out[f"ind{t}"], out[f"mask{t}"], out[f"anno_box{t}"] = ind, mask, anno
    return out


# ---- mmdet 2.x, restated ------------------------------------------------------------------------------------------------------------
def _mmdet():
    import torch
    import torch.nn.functional as F

    def weight_reduce_loss(loss, weight=None, reduction="mean", avg_factor=None):
        if weight is not None:
            loss = loss * weight
        if avg_factor is None:
            return loss.mean() if reduction == "mean" else (loss.sum() if reduction == "sum" else loss)
        if reduction == "mean":
            return loss.sum() / avg_factor
        if reduction != "none":
            raise ValueError('avg_factor can not be used with reduction="sum"')
        return loss

    def gaussian_focal_loss(pred, gaussian_target, weight=None, alpha=2.0, gamma=4.0, reduction="mean", avg_factor=None):
        eps = 1e-12
        pos_weights = gaussian_target.eq(1)
        neg_weights = (1 - gaussian_target).pow(gamma)
        pos_loss = -(pred + eps).log() * (1 - pred).pow(alpha) * pos_weights
        neg_loss = -(1 - pred + eps).log() * pred.pow(alpha) * neg_weights
        return weight_reduce_loss(pos_loss + neg_loss, weight, reduction, avg_factor)

    def py_sigmoid_focal_loss(pred, target, weight=None, gamma=2.0, alpha=0.25, reduction="mean", avg_factor=None):
        pred_sigmoid = pred.sigmoid()
        target = target.type_as(pred)
        pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
        focal_weight = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
        loss = F.binary_cross_entropy_with_logits(pred, target, reduction="none") * focal_weight
        if weight is not None:
            if weight.shape != loss.shape:
                if weight.size(0) == loss.size(0):
                    weight = weight.view(-1, 1)
                else:
                    weight = weight.view(loss.size(0), -1)
        return weight_reduce_loss(loss, weight, reduction, avg_factor)

    def l1_loss(pred, target, weight=None, reduction="mean", avg_factor=None):
        if target.numel() == 0:
            return pred.sum() * 0
        return weight_reduce_loss(torch.abs(pred - target), weight, reduction, avg_factor)

    class GaussianFocalLoss:
        def __init__(self, alpha=2.0, gamma=4.0, reduction="mean", loss_weight=1.0):
            self.alpha, self.gamma, self.reduction, self.loss_weight = alpha, gamma, reduction, loss_weight

        def __call__(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
            return self.loss_weight * gaussian_focal_loss(pred, target, weight, alpha=self.alpha, gamma=self.gamma,
                                                          reduction=reduction_override or self.reduction, avg_factor=avg_factor)

    class FocalLoss:
        def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0):
            assert use_sigmoid is True
            self.gamma, self.alpha, self.reduction, self.loss_weight = gamma, alpha, reduction, loss_weight

        def __call__(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
            num_classes = pred.size(1)
            target = F.one_hot(target, num_classes=num_classes + 1)[:, :num_classes]
            return self.loss_weight * py_sigmoid_focal_loss(pred, target, weight, gamma=self.gamma, alpha=self.alpha,
                                                            reduction=reduction_override or self.reduction, avg_factor=avg_factor)

    class L1Loss:
        def __init__(self, reduction="mean", loss_weight=1.0):
            self.reduction, self.loss_weight = reduction, loss_weight

        def __call__(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
            return self.loss_weight * l1_loss(pred, target, weight, reduction=reduction_override or self.reduction, avg_factor=avg_factor)

    return dict(GaussianFocalLoss=GaussianFocalLoss, FocalLoss=FocalLoss, L1Loss=L1Loss)


def _lines(rel, first, last, sentinel):
    path = os.path.join(REF, rel)
    src = textwrap.dedent("\n".join(open(path).read().split("\n")[first - 1:last]))
    assert src.split("\n")[0].strip().startswith(sentinel), (rel, first, src.split("\n")[0])
    return src, path


def _load_cfg():
    import yaml

    out = {}
    for head, keys in (("transfusion", ("loss_cls", "loss_heatmap", "loss_bbox")), ("centerhead", ("loss_cls", "loss_bbox"))):
        cfg = yaml.safe_load(open(os.path.join(REF, "configs/nuscenes/det", head, "default.yaml")))
        obj = cfg["model"]["heads"]["object"]
        out[head] = {k: obj[k] for k in keys}
    return out


def _build(block, classes):
    block = dict(block)
    return classes[block.pop("type")](**block)


def reference():
    """-> (transfusion_loss(self, preds_dicts, targets...), centerhead_loss(self, preds_dicts, heatmaps, ...), the loss configs)."""
    import torch

    ns_tf = dict(torch=torch)
    src, path = _lines("mmdet3d/models/heads/bbox/transfusion.py", 31, 33, "def clip_sigmoid")
    exec(compile(src, path, "exec"), ns_tf)
    body, path = _lines("mmdet3d/models/heads/bbox/transfusion.py", 612, 711, "preds_dict = preds_dicts[0][0]")
    exec(compile("def loss(self, preds_dicts, labels, label_weights, bbox_targets, bbox_weights, ious, num_pos, matched_ious, heatmap):\n"
                 + textwrap.indent(body, "    ") + "\n    return loss_dict\n", path, "exec"), ns_tf)
    ns_ch = dict(torch=torch)
    src, path = _lines("mmdet3d/models/heads/bbox/centerpoint.py", 15, 16, "def clip_sigmoid")
    exec(compile(src, path, "exec"), ns_ch)
    src, path = _lines("mmdet3d/models/heads/bbox/centerpoint.py", 368, 388, "def _gather_feat")
    exec(compile(src, path, "exec"), ns_ch)
    body, path = _lines("mmdet3d/models/heads/bbox/centerpoint.py", 597, 633, "for task_id, preds_dict in enumerate(preds_dicts):")
    exec(compile("def loss(self, preds_dicts, heatmaps, anno_boxes, inds, masks):\n    loss_dict = dict()\n"
                 + textwrap.indent(body, "    ") + "\n    return loss_dict\n", path, "exec"), ns_ch)
    return ns_tf["loss"], ns_ch["loss"], ns_ch["_gather_feat"], _load_cfg()


def _run_tf(loss_fn, cfg, name, dtype):
    import torch

    c, inp, classes = TF_CASES[name], tf_inputs(name), _mmdet()
    names = ["dense_heatmap", "heatmap"] + [n for n, _ in PIECES[:5 if c["D"] == 10 else 4]]
    leaves = {n: torch.from_numpy(inp[n]).to(dtype).requires_grad_(True) for n in names}
    preds = {n: v * 1 for n, v in leaves.items()}                                # clip_sigmoid works in place: no leaf may be handed in
    self = types.SimpleNamespace(num_decoder_layers=c["L"], auxiliary=True, num_proposals=c["K"], num_classes=c["C"],
                                 train_cfg=dict(code_weights=CODE_WEIGHTS[:c["D"]]), loss_heatmap=_build(cfg["loss_heatmap"], classes),
                                 loss_cls=_build(cfg["loss_cls"], classes), loss_bbox=_build(cfg["loss_bbox"], classes))
    losses = loss_fn(self, [[preds]], torch.from_numpy(inp["labels"]), torch.from_numpy(inp["label_weights"]),
                     torch.from_numpy(inp["bbox_targets"]).to(dtype), torch.from_numpy(inp["bbox_weights"]).to(dtype), None,
                     int(inp["num_pos"]), float(inp["matched_ious"]), torch.from_numpy(inp["heatmap_target"]).to(dtype))
    sum(v for k, v in losses.items() if k != "matched_ious").backward()
    num_pos = {"heat": float((inp["heatmap_target"] == 1).sum())}
    return ({k: v.detach().numpy().astype(np.float64) for k, v in losses.items()},
            {n: v.grad.numpy().astype(np.float64) for n, v in leaves.items()}, num_pos, inp)


def _run_ch(loss_fn, gather, cfg, name, dtype):
    import torch

    c, inp, classes = CH_CASES[name], ch_inputs(name), _mmdet()
    T = len(c["classes"])
    names = [f"{n}{t}" for t in range(T) for n in ("heatmap",) + tuple(p for p, _ in CH_PIECES)]
    leaves = {n: torch.from_numpy(inp[n]).to(dtype).requires_grad_(True) for n in names}
    preds = [[{n: leaves[f"{n}{t}"] * 1 for n in ("heatmap",) + tuple(p for p, _ in CH_PIECES)}] for t in range(T)]
    self = types.SimpleNamespace(train_cfg=dict(code_weights=CODE_WEIGHTS), loss_cls=_build(cfg["loss_cls"], classes),
                                 loss_bbox=_build(cfg["loss_bbox"], classes))
    self._gather_feat = types.MethodType(gather, self)
    losses = loss_fn(self, preds, [torch.from_numpy(inp[f"heatmap_target{t}"]).to(dtype) for t in range(T)],
                     [torch.from_numpy(inp[f"anno_box{t}"]).to(dtype) for t in range(T)], [torch.from_numpy(inp[f"ind{t}"]) for t in range(T)],
                     [torch.from_numpy(inp[f"mask{t}"]) for t in range(T)])
    sum(losses.values()).backward()
    num_pos = {f"heat{t}": float((inp[f"heatmap_target{t}"] == 1).sum()) for t in range(T)}
    return ({k: v.detach().numpy().astype(np.float64) for k, v in losses.items()},
            {n: v.grad.numpy().astype(np.float64) for n, v in leaves.items()}, num_pos, inp)


def main():
    import torch

    torch.set_num_threads(1)
    tf_loss, ch_loss, gather, cfg = reference()
    store = {f"cfg/{k}": np.array(json.dumps(v)) for k, v in cfg.items()}
    runs = [(n, lambda dt, n=n: _run_tf(tf_loss, cfg["transfusion"], n, dt)) for n in TF_CASES]
    runs += [(n, lambda dt, n=n: _run_ch(ch_loss, gather, cfg["centerhead"], n, dt)) for n in CH_CASES]
    for name, run in runs:
        loss64, grad64, num_pos, inp = run(torch.float64)
        loss32, grad32, _, _ = run(torch.float32)
        for k, v in inp.items():
            store[f"{name}/in/{k}"] = v
        for k, v in num_pos.items():
            store[f"{name}/num_pos/{k}"] = np.float64(v)
        for k in loss64:
            store[f"{name}/loss/{k}"] = loss64[k]
            store[f"{name}/err_loss/{k}"] = np.float64(np.max(np.abs(loss32[k] - loss64[k])))
        for k in grad64:
            store[f"{name}/grad/{k}"] = grad64[k]
            store[f"{name}/err_grad/{k}"] = np.float64(np.max(np.abs(grad32[k] - grad64[k])))
        print(name, {k: (float(v), float(store[f"{name}/err_loss/{k}"])) for k, v in loss64.items()})
    assert store["ch_tasks/loss/bbox/task2"] == 0.0
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
