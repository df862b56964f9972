"""CPU: the head losses' host formulation against tests/golden/head_losses_ref.npz (the REFERENCE's TransFusionHead.loss and
CenterHead.loss statements on CPU torch in float64, see tests/golden/make_head_losses_golden.py), the loss registry against the
loss blocks of both head configs, and the host-only parts of the C ABI: the plan and the argument checks."""
import ctypes
import json
import os
from ctypes import c_size_t, c_void_p

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi, head_losses, heads
from bevfusion_amd.registry import LOSSES

HERE = os.path.dirname(os.path.abspath(__file__))
TF = {"tf_small": (3, 17, 3), "tf_empty": (2, 5, 3), "tf_one_layer": (1, 17, 3)}     # fixture -> (layers, proposals, classes)
CH = {"ch_tasks": 3}
TF_PREDS = ("dense_heatmap", "heatmap", "center", "height", "dim", "rot", "vel")
CH_PREDS = ("heatmap", "reg", "height", "dim", "rot", "vel")
NEW = ["bevamd_head_loss_plan", "bevamd_gaussian_focal_forward", "bevamd_gaussian_focal_backward",
       "bevamd_transfusion_layer_losses_forward", "bevamd_transfusion_layer_losses_backward", "bevamd_centerhead_box_loss_forward",
       "bevamd_centerhead_box_loss_backward"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "head_losses_ref.npz")))


def inputs(gold, name):
    return {k.split("/in/")[1]: v for k, v in gold.items() if k.startswith(name + "/in/")}


def tf_call(gold, name, dtype=torch.float64, device="cpu", sync_free=False):
    """-> (loss dict, leaves by name) of transfusion_loss on the fixture."""
    layers, K, C = TF[name]
    i = inputs(gold, name)
    leaves = {n: torch.from_numpy(i[n]).to(dtype).to(device).requires_grad_(True) for n in TF_PREDS if n in i}
    num_pos, ious = int(i["num_pos"]), float(i["matched_ious"])
    if sync_free:
        num_pos = torch.full((), num_pos, dtype=torch.int32, device=device)
        ious = torch.full((), ious, dtype=torch.float32, device=device)
    targets = (torch.from_numpy(i["labels"]).to(device), torch.from_numpy(i["label_weights"]).to(device),
               torch.from_numpy(i["bbox_targets"]).to(device), torch.from_numpy(i["bbox_weights"]).to(device), None, num_pos, ious,
               torch.from_numpy(i["heatmap_target"]).to(device))
    code_weights = head_losses._DEFAULT_CODE_WEIGHTS
    return heads.transfusion_loss(leaves, targets, K, C, layers, code_weights=code_weights), leaves


def ch_call(gold, name, dtype=torch.float64, device="cpu"):
    T = CH[name]
    i = inputs(gold, name)
    leaves = [{n: torch.from_numpy(i[f"{n}{t}"]).to(dtype).to(device).requires_grad_(True) for n in CH_PREDS} for t in range(T)]
    classes = [i[f"heatmap{t}"].shape[1] for t in range(T)]
    B, S = i["heatmap0"].shape[0], i["heatmap0"].shape[2]
    # the heatmaps as centerhead_get_targets hands them out: views into ONE buffer, so later tasks' bases are 4-byte aligned only
    flat = torch.cat([torch.from_numpy(i[f"heatmap_target{t}"]).reshape(-1) for t in range(T)]).to(device)
    heatmaps, base = [], 0
    for c in classes:
        heatmaps.append(flat[base:base + B * c * S * S].view(B, c, S, S))
        base += B * c * S * S
    targets = (heatmaps, [torch.from_numpy(i[f"anno_box{t}"]).to(device) for t in range(T)],
               [torch.from_numpy(i[f"ind{t}"]).to(device) for t in range(T)], [torch.from_numpy(i[f"mask{t}"]).to(device) for t in range(T)])
    return heads.centerhead_loss([[d] for d in leaves], targets), {f"{n}{t}": v for t, d in enumerate(leaves) for n, v in d.items()}


def total(losses):
    return sum(v for k, v in losses.items() if k != "matched_ious")


def close(got, want, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() <= rel * max(np.abs(want).max(), 1e-300) or (not want.any() and not got.any())


@pytest.mark.parametrize("name", list(TF) + list(CH))
def test_host_formulation_reproduces_the_reference_in_float64(gold, name):
    losses, leaves = tf_call(gold, name) if name in TF else ch_call(gold, name)
    total(losses).backward()
    keys = [k.split("/loss/")[1] for k in gold if k.startswith(name + "/loss/")]
    assert sorted(keys) == sorted(losses)
    for k in keys:
        assert close(losses[k].detach().numpy(), gold[f"{name}/loss/{k}"]), k
    grads = [k.split("/grad/")[1] for k in gold if k.startswith(name + "/grad/")]
    assert sorted(grads) == sorted(leaves)
    for k in grads:
        assert close(leaves[k].grad.numpy(), gold[f"{name}/grad/{k}"]), k


def test_fixtures_hold_the_cases_they_are_for(gold):
    i = inputs(gold, "tf_small")
    t, x = i["heatmap_target"], i["dense_heatmap"]
    assert t.size == 726 and t.size % 4 and t.size < head_losses.head_loss_plan(t.size)[1]
    assert (t == 1).sum() >= 3 and (t == np.nextafter(np.float32(1), np.float32(0))).sum() == 3 and (np.abs(x) == 12).sum() >= 4
    assert not gold["tf_small/grad/dense_heatmap"][np.abs(x) == 12].any()          # the clamp is active: exactly 0
    assert (i["labels"] == 3).any() and (i["label_weights"] == 0).any() and i["num_pos"] > 0
    e = inputs(gold, "tf_empty")
    assert not (e["heatmap_target"] == 1).any() and e["num_pos"] == 0
    assert "vel" not in inputs(gold, "tf_one_layer") and inputs(gold, "tf_one_layer")["bbox_targets"].shape[2] == 8
    c = inputs(gold, "ch_tasks")
    assert [c[f"heatmap{t}"].shape[1] for t in range(3)] == [1, 2, 2] and (c["heatmap0"][0, 0].size * 4) % 16
    assert c["ind0"][0, 0] == c["ind0"][0, 1] and c["mask0"][0, :2].all() and not c["mask0"].all()
    assert not c["mask2"].any() and gold["ch_tasks/loss/bbox/task2"] == 0 and gold["ch_tasks/num_pos/heat2"] == 0


def test_loss_blocks_of_both_head_configs_build(gold):
    """configs/nuscenes/det/{transfusion,centerhead}/default.yaml: loss_cls / loss_heatmap / loss_bbox, recorded by the maker."""
    want = {"transfusion": dict(loss_cls=heads.FocalLoss, loss_heatmap=heads.GaussianFocalLoss, loss_bbox=heads.L1Loss),
            "centerhead": dict(loss_cls=heads.GaussianFocalLoss, loss_bbox=heads.L1Loss)}
    for head, blocks in want.items():
        cfg = json.loads(str(gold[f"cfg/{head}"]))
        assert sorted(cfg) == sorted(blocks)
        for key, cls in blocks.items():
            module = LOSSES.build(cfg[key])
            assert type(module) is cls and module.reduction == "mean"
            assert module.loss_weight == cfg[key].get("loss_weight", 1.0)
    tf = json.loads(str(gold["cfg/transfusion"]))
    losses, _ = tf_call(gold, "tf_one_layer")
    layers, K, C = TF["tf_one_layer"]
    i = inputs(gold, "tf_one_layer")
    again = heads.transfusion_loss(
        {n: torch.from_numpy(i[n]).double() for n in TF_PREDS if n in i},
        (torch.from_numpy(i["labels"]), torch.from_numpy(i["label_weights"]), torch.from_numpy(i["bbox_targets"]),
         torch.from_numpy(i["bbox_weights"]), None, int(i["num_pos"]), float(i["matched_ious"]), torch.from_numpy(i["heatmap_target"])),
        K, C, layers, **tf)
    assert all(torch.equal(losses[k].detach(), again[k]) for k in losses)
    assert heads.LOSSES is LOSSES and "FocalLoss" in LOSSES


def test_loss_modules_on_host_tensors():
    g = torch.Generator().manual_seed(5)
    p = torch.rand(3, 7, generator=g, dtype=torch.float64) * 0.98 + 0.01
    t = torch.rand(3, 7, generator=g, dtype=torch.float64)
    t[0, 0] = 1
    want = head_losses._gaussian_focal_host(p, t).sum()
    assert torch.equal(heads.GaussianFocalLoss(loss_weight=0.5)(p, t, avg_factor=4), 0.5 * (want / 4))
    assert torch.equal(heads.GaussianFocalLoss(reduction="sum")(p, t), want / 1.0)
    assert torch.equal(heads.GaussianFocalLoss()(p, t, avg_factor=torch.tensor(2.0)), want / 2.0)
    x = torch.randn(5, 3, generator=g, dtype=torch.float64)
    y = torch.tensor([0, 3, 2, 3, 1])
    w = torch.tensor([1, 1, 0, 2, 1])
    focal = head_losses._sigmoid_focal_host(x, y, w).sum()
    assert torch.equal(heads.FocalLoss()(x, y, w, avg_factor=3), focal / 3.0)
    assert torch.equal(heads.FocalLoss()(x, y, w), focal / 15.0)                   # the mean over N x C elements
    a, b = torch.randn(4, 8, generator=g), torch.randn(4, 8, generator=g)
    assert torch.equal(heads.L1Loss(loss_weight=0.25)(a, b, torch.ones_like(a), avg_factor=2), 0.25 * ((a - b).abs().sum() / 2))
    with pytest.raises(NotImplementedError):
        heads.GaussianFocalLoss()(p, t, reduction_override="none")
    with pytest.raises(NotImplementedError):
        heads.FocalLoss(use_sigmoid=False)
    with pytest.raises(NotImplementedError):
        heads.transfusion_loss({"dense_heatmap": p, "heatmap": x}, None, 1, 3, loss_cls=dict(type="L1Loss"))


def test_plan_answers_without_a_device():
    share = head_losses.head_loss_plan(1)[1]
    assert share >= 256 and share % 4 == 0
    assert [head_losses.head_loss_plan(n) for n in (1, share, share + 1)] == [(1, share), (1, share), (2, share)]
    groups, s = head_losses.head_loss_plan(2 ** 31)
    assert s == share and 1 <= groups < (2 ** 31) // share                          # the grid cap: several passes per workgroup
    assert head_losses.head_loss_plan(groups * share + 1)[0] == groups
    lib = _capi.load()
    assert lib.bevamd_head_loss_plan(0, (ctypes.c_int * 2)()) == 1 and "cells" in _capi.last_error()
    assert lib.bevamd_head_loss_plan(5, None) == 1


def test_bad_arguments_are_refused_before_any_gpu_work():
    lib = _capi.load()
    one = (ctypes.c_void_p * 17)(*([8] * 17))          # non-null addresses that are never dereferenced: every call fails its checks
    cells = (ctypes.c_longlong * 17)(*([4] * 17))
    cw = (ctypes.c_float * 10)(*([1.0] * 10))
    x = ctypes.c_void_p(8)
    assert lib.bevamd_gaussian_focal_forward(one, one, cells, 17, 1, 2.0, 4.0, 1.0, None, x, x, x, None) == 1
    assert "17 maps" in _capi.last_error()
    assert lib.bevamd_gaussian_focal_forward(None, one, cells, 1, 1, 2.0, 4.0, 1.0, None, x, x, x, None) == 1
    assert lib.bevamd_gaussian_focal_forward(one, one, cells, 1, 1, 2.0, 4.0, 1.0, None, None, x, x, None) == 1
    assert "null" in _capi.last_error()
    assert lib.bevamd_gaussian_focal_backward(one, one, cells, 2, 1, 2.0, 4.0, 1.0, None, x, x, None, None) == 1
    layer = lambda scores, dtype, center, vel, D, num_pos=x: lib.bevamd_transfusion_layer_losses_forward(   # noqa: E731
        scores, x, x, dtype, center, x if center else None, x if center else None, x if center else None, vel, x, x, cw, num_pos, None, None,
        2, 3, 1, 4, D, 0.25, 2.0, 1.0, 0.25, x, x, None)
    assert layer(x, 0, x, x, 9) == 1 and "8 or 10 columns" in _capi.last_error()
    assert layer(x, 0, x, None, 10) == 1                                         # ten columns need vel
    assert layer(x, 1, x, x, 10) == 4 and "dtype" in _capi.last_error()
    assert layer(None, 0, None, None, 10) == 1
    assert layer(x, 0, x, x, 10, num_pos=None) == 1
    box = lambda T, M, maps=one: lib.bevamd_centerhead_box_loss_forward(maps, one, one, one, T, 2, M, 169, cw, 0.25, x, x, None)   # noqa: E731
    maps = (ctypes.c_void_p * 85)(*([8] * 85))
    assert box(17, 9, maps) == 1 and "17 tasks" in _capi.last_error()
    assert box(1, 1025, maps) == 4 and "max_objs" in _capi.last_error()
    assert box(1, 9, None) == 1
    assert lib.bevamd_centerhead_box_loss_backward(maps, one, one, one, 1, 2, 9, 169, cw, 0.25, x, x, None, None) == 1


def test_new_entry_points_take_no_pointer_with_a_byte_count():
    for name in NEW:
        args = _capi._EXT_SIGNATURES[name][1]
        assert not any(a is c_void_p and b is c_size_t for a, b in zip(args, args[1:])) and c_size_t not in args, name


def test_device_ops_refuse_host_tensors_and_fp16():
    z = torch.zeros(1, 2, 4)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        head_losses.gaussian_focal_forward([z], [z])
    with pytest.raises(RuntimeError, match="GPU tensors"):
        head_losses.transfusion_layer_losses_forward(z, torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4), None, None, None, None, None)
