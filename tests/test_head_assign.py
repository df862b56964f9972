"""CPU: the TransFusion assignment (bevfusion_amd/head_assign.py over csrc/ext/head_assign.hip) against
tests/golden/head_assign_ref.npz (the REFERENCE's own assigner, overlaps, coder and get_targets_single statements on CPU torch with
scipy's solver, see tests/golden/make_head_assign_golden.py): the fixture's inputs, the numpy host mirror `_targets_host`, the
registries, the argument errors and the C-ABI symbols.  `check_targets` carries the bars for this file and for
tests/test_gpu_head_assign.py.

Bars, derived.  Assignment, labels, label_weights, bbox_weights, num_pos: equal (every row-wise fixture has a unique optimum with
margin `margin` >= 1e-3, and the callers assert that their cost error cannot bridge it: 2 * min(K, G) * bar < margin).  bbox_targets:
columns 0, 1, 2, 8, 9 bit-equal (the same correctly rounded fp32 operations), log / sin / cos within 1 ulp of the fixture's float64
value rounded to fp32.  ious and matched_ious within the caller's iou bar.  The host mirror's own bars: its BEV overlap IS the
oracle's, as in the fixture, so iou is held to 2 ulp at 1 (2.4e-7: the volume products may associate differently); cost sums three
terms of magnitude below 2 (focal <= 0.15 * 0.75 * 12, L1 <= 0.5, iou <= 0.25), each at most 8 fp32 roundings away from the
reference's order of evaluation: 8 * 2^-24 * 2 = 9.5e-7, doubled: 2e-6."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import oracle
from bevfusion_amd import _capi, head_assign, heads
from bevfusion_amd.registry import BBOX_ASSIGNERS, MATCH_COST

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_head_assign_golden", os.path.join(HERE, "golden", "make_head_assign_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = list(gen.CASES)
ROWWISE = list(gen.ROWWISE)
MIRROR_COST_BAR = 2e-6
MIRROR_IOU_BAR = 2.4e-7


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "head_assign_ref.npz")))


def make_assigner(case):
    return BBOX_ASSIGNERS.build(gen.assigner_cfg(case))


def make_coder(case):
    return heads.TransFusionBBoxCoder(**gen.coder_kwargs(case))


def cls_spec(case):
    w = gen.WEIGHTS
    return ("softmax", w["cls"]) if gen.CASES[case].get("cls") == "softmax" else ("focal", w["cls"], w["alpha"], w["gamma"], 1e-12)


def bev_overlap(a, b):
    return oracle.iou3d_pairwise(a, b, "overlap")


def host_mirror(case, col4row=None, iou=None, boxes=None):
    """`_targets_host` on the fixture's inputs (boxes: the decoded boxes to use; default: the host decode)."""
    c = gen.CASES[case]
    d = gen.inputs(case)
    coder = make_coder(case)
    if boxes is None:
        p = {k: torch.from_numpy(v) for k, v in d["preds"].items()}
        boxes = heads._decode_host(p["heatmap"], p["rot"], p["dim"], p["center"], p["height"], p.get("vel"), coder)[0].numpy()
    gt_boxes, gt_labels, offsets = gen.packed(case)
    return head_assign._targets_host(
        boxes, d["preds"]["heatmap"], gt_boxes, gt_labels, offsets, c["L"], c["K"], cls_spec(case), gen.WEIGHTS["reg"], gen.WEIGHTS["iou"],
        gen.PC_RANGE, head_assign._coder_consts(coder), gen.C, gen.code_size(case), gen.case_cfg(case)["pos_weight"], bev_overlap,
        col4row=col4row, iou=iou)


def check_targets(case, gold, got, iou_bar):
    """labels, label_weights, bbox_targets, bbox_weights, ious, num_pos, matched_ious of a row-wise fixture against the golden."""
    p = case + "."
    for name in ("labels", "label_weights", "bbox_weights"):
        a = np.asarray(got[name])
        assert a.dtype == gold[p + name].dtype and np.array_equal(a, gold[p + name]), name
    assert int(got["num_pos"]) == int(gold[p + "num_pos"])
    t = np.asarray(got["bbox_targets"])
    code = t.shape[-1]
    exact = [0, 1, 2] + ([8, 9] if code == 10 else [])
    assert t.dtype == np.float32 and np.array_equal(t[..., exact].view(np.int32), gold[p + "bbox_targets"][..., exact].view(np.int32))
    assert gen.ulps(t[..., 3:8], gold[p + "bbox_targets64"][..., 3:8]).max() <= 1
    err = np.abs(np.asarray(got["ious"], np.float64) - gold[p + "ious"]).max()
    mean_err = abs(float(got["matched_ious"]) - float(gold[p + "matched_ious"]))
    assert err <= iou_bar and mean_err <= iou_bar + 6e-8, (err, mean_err, iou_bar)   # + half an fp32 ulp below 1: the stored mean is fp32
    return err, mean_err


def cost_errors(case, gold, cost, iou):
    """Largest absolute error of cost / iou [B, L, K, Gmax] against the golden over the live entries."""
    c = gen.CASES[case]
    worst_c = worst_i = 0.0
    for b, G in enumerate(c["G"]):
        if G:
            worst_c = max(worst_c, float(np.abs(cost[b, :, :, :G].astype(np.float64) - gold[case + ".cost"][b, :, :, :G]).max()))
            worst_i = max(worst_i, float(np.abs(iou[b, :, :, :G].astype(np.float64) - gold[case + ".iou"][b, :, :, :G]).max()))
    return worst_c, worst_i


def margin_admits(case, gold, cost_bar):
    """The inequality that makes the golden's unique optimum the optimum on costs within cost_bar of it."""
    c = gen.CASES[case]
    side = max(min(c["K"], G) for G in c["G"])
    return 2 * side * cost_bar < float(gold[case + ".margin"])


@pytest.mark.parametrize("case", CASES)
def test_stored_digests_match_the_inputs(case, gold):
    assert gen.digest(case) == str(gold[case + ".inputs_sha256"])
    d = gen.inputs(case)
    c = gen.CASES[case]
    assert d["preds"]["heatmap"].shape == (c["B"], gen.C, c["L"] * c["K"]) and np.abs(d["preds"]["heatmap"]).max() <= 12
    assert [len(l) for l in d["gt_labels"]] == list(c["G"])


@pytest.mark.parametrize("case", ROWWISE)
def test_fixtures_have_a_unique_optimum(case, gold):
    assert float(gold[case + ".margin"]) >= gen.DELTA and margin_admits(case, gold, MIRROR_COST_BAR)


@pytest.mark.parametrize("case", ROWWISE)
def test_host_mirror_reproduces_the_reference(case, gold):
    c = gen.CASES[case]
    out = host_mirror(case)
    gmax = gold[case + ".cost"].shape[-1]
    cost = np.zeros((c["B"], c["L"], c["K"], gmax), np.float32)
    iou = np.zeros_like(cost)
    it = iter(zip(out["cost"], out["iou"]))
    for b, G in enumerate(c["G"]):
        for l in range(c["L"] if G else 0):
            cost[b, l, :, :G], iou[b, l, :, :G] = next(it)
    ec, ei = cost_errors(case, gold, cost, iou)
    print(f"{case}: host mirror cost error {ec:.3e} (bar {MIRROR_COST_BAR}), iou error {ei:.3e} (bar {MIRROR_IOU_BAR})")
    assert ec <= MIRROR_COST_BAR and ei <= MIRROR_IOU_BAR
    assert np.array_equal(out["col4row"], gold[case + ".col4row"])
    check_targets(case, gold, out, MIRROR_IOU_BAR)
    assert not out["flags"].any()


def test_host_mirror_config_shape_totals(gold):
    """K = 200 against 40, 120, 7 and 260 boxes: no unique optimum, so only the totals are compared (at min(K, G) entries of error)."""
    case = "config_shape"
    c = gen.CASES[case]
    out = host_mirror(case)
    assert out["num_pos"] == int(gold[case + ".num_pos"]) == sum(min(c["K"], G) for G in c["G"])
    for n, (cost, G) in enumerate(zip(out["cost"], c["G"])):
        c4r = out["col4row"][n]
        rows = np.nonzero(c4r >= 0)[0]
        total = cost[rows, c4r[rows]].astype(np.float64).sum()
        assert abs(total - gold[case + ".totals"][n]) <= min(c["K"], G) * MIRROR_COST_BAR


def test_registries_build_the_config_block():
    cfg = dict(type="HungarianAssigner3D", iou_calculator=dict(type="BboxOverlaps3D", coordinate="lidar"),
               cls_cost=dict(type="FocalLossCost", gamma=2.0, alpha=0.25, weight=0.15), reg_cost=dict(type="BBoxBEVL1Cost", weight=0.25),
               iou_cost=dict(type="IoU3DCost", weight=0.25))
    a = BBOX_ASSIGNERS.build(cfg)
    assert isinstance(a, heads.HungarianAssigner3D) and isinstance(a.cls_cost, heads.FocalLossCost) and a.cls_cost.weight == 0.15
    assert a.cls_cost.gamma == 2.0 and a.reg_cost.weight == 0.25 and a.iou_cost.weight == 0.25 and a.iou_calculator.coordinate == "lidar"
    d = heads.HungarianAssigner3D()                                            # the constructor's defaults
    assert type(d.cls_cost) is heads.ClassificationCost and d.cls_cost.weight == 1.0 and d.reg_cost.weight == 1.0
    assert MATCH_COST.get("IoU3DCost") is heads.IoU3DCost and "ClassificationCost" in MATCH_COST
    with pytest.raises(NotImplementedError, match="HeuristicAssigner"):
        BBOX_ASSIGNERS.build(dict(type="HeuristicAssigner3D", dist_thre=100))
    with pytest.raises(NotImplementedError, match="LiDAR"):
        heads.BboxOverlaps3D(coordinate="camera")


def test_argument_errors():
    case = "small"
    c = gen.CASES[case]
    d = gen.inputs(case)
    preds = {k: torch.from_numpy(v) for k, v in d["preds"].items()}
    boxes = [torch.from_numpy(b) for b in d["gt_boxes"]]
    labels = [torch.from_numpy(l) for l in d["gt_labels"]]
    args = (preds, make_coder(case), make_assigner(case))
    with pytest.raises(RuntimeError, match="GPU tensors"):                   # no CPU path
        heads.transfusion_get_targets(boxes, labels, *args, gen.case_cfg(case), c["K"], gen.C)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        heads.linear_sum_assignment_batch(torch.zeros((2, 3, 3)))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        make_assigner(case).assign(torch.zeros((4, 7)), boxes[0], labels[0], torch.zeros((1, gen.C, 4)), gen.case_cfg(case))
    with pytest.raises(ValueError, match="pos_weight"):
        heads.transfusion_get_targets(boxes, labels, *args, dict(gen.case_cfg(case), pos_weight=1.5), c["K"], gen.C)
    with pytest.raises(NotImplementedError, match="HungarianAssigner3D"):
        heads.transfusion_get_targets(boxes, labels, preds, make_coder(case), object(), gen.case_cfg(case), c["K"], gen.C)
    with pytest.raises(ValueError, match="num_proposals"):
        heads.transfusion_get_targets(boxes, labels, *args, gen.case_cfg(case), 1025, gen.C)


def test_symbols_are_declared_and_bound():
    root = os.path.dirname(HERE)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "bevfusion_amd_ext.h")).read(), flags=re.S)
    ext = ctypes.CDLL(_capi.EXT_LIB_PATH)
    for name in ("bevamd_match_costs", "bevamd_linear_sum_assignment", "bevamd_transfusion_assign_targets"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _capi.ext_exported_names() and hasattr(ext, name)


def test_library_rejects_sizes_over_the_limits_before_any_gpu_work():
    lib = _capi.load()
    rc = lib.bevamd_linear_sum_assignment(None, None, None, 1, 1025, 8, None, None, None)
    assert rc == 4 and "1024" in _capi.last_error()
    rc = lib.bevamd_linear_sum_assignment(None, None, None, 1, 8, 1025, None, None, None)
    assert rc == 4
    rc = lib.bevamd_match_costs(None, None, None, None, None, 0, 7, 1, 1, 16, 10, 1025, 1, 0.15, 0.25, 2.0, 1e-12, 1, 0.25, 1, 0.25, None,
                                None, None, None, None, None)
    assert rc == 4 and "max_boxes_per_sample" in _capi.last_error()
    rc = lib.bevamd_match_costs(None, None, None, None, None, 0, 7, 1, 1, 1025, 10, 16, 1, 0.15, 0.25, 2.0, 1e-12, 1, 0.25, 1, 0.25, None,
                                None, None, None, None, None)
    assert rc == 4 and "proposals" in _capi.last_error()
    rc = lib.bevamd_transfusion_assign_targets(None, None, None, None, None, None, None, 0, 7, 1, 1, 16, 16, 10, 10, -1, None, None, None,
                                               None, None, None, None, None, None, None)
    assert rc == 1 and "code_size" in _capi.last_error()
