"""CPU: the head training targets (bevfusion_amd/head_targets.py over csrc/ext/head_targets.hip) against
tests/golden/head_targets_ref.npz (the REFERENCE's own target code on CPU torch, see tests/golden/make_head_targets_golden.py):
the fixture's inputs, the numpy host mirror `_targets_host`, the argument errors and the C-ABI symbols.  `check_case` carries the
bars for this file and for tests/test_gpu_head_targets.py.

Bars, derived: ind, mask and overflow equal; anno_box columns 0, 1, 2, 8, 9 and raw dims bit-equal (the same correctly rounded fp32
operations in the same order); log / sin / cos within 1 ulp of the fixture's float64 value rounded to fp32 (a double evaluation that
is off by one double ulp can only move a rounding tie), hence within 2 ulp of the reference's fp32; heatmap cells that are 0 or 1.0
in the golden equal (num_pos is eq(1)), every other cell within 1 fp32 ulp (one rounding of a double evaluation)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi, head_targets, heads

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_head_targets_golden", os.path.join(HERE, "golden", "make_head_targets_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = list(gen.CASES)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "head_targets_ref.npz")))


def golden_heatmaps(case, gold):
    """-> (per task [B, C_t, size, size], the TransFusion variant's [B, C, size, size])."""
    c = gen.CASES[case]
    count = gen.B * sum(c["classes"]) * c["size"] ** 2
    flat = gen.dense_heatmap(gold[case + ".heatmap_idx"], gold[case + ".heatmap_val"], count)
    tf = gen.dense_heatmap(gold[case + ".tf_heatmap_idx"], gold[case + ".tf_heatmap_val"], count)
    return gen.split_heatmaps(flat, c["classes"], c["size"]), tf.reshape(gen.B, sum(c["classes"]), c["size"], c["size"])


def check_heatmap(got, want):
    """-> the number of cells that are not bit-equal (after the bars)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    pinned = (want == 0) | (want == 1)
    assert np.array_equal(got[pinned], want[pinned]), "cells that are 0 or 1.0 in the golden differ"
    u = gen.ulps(got[~pinned], want[~pinned])
    assert u.max(initial=0) <= 1, f"heatmap off by {u.max()} ulp"
    return int((got.view(np.int32) != want.view(np.int32)).sum())


def check_case(case, gold, heatmaps, anno, ind, mask, overflow):
    """CenterHead outputs of a case (numpy, per task) against the golden -> heatmap cells that are not bit-equal."""
    c = gen.CASES[case]
    p = case + "."
    anno, ind, mask = np.stack(anno), np.stack(ind), np.stack(mask)
    assert anno.dtype == np.float32 and ind.dtype == np.int64 and mask.dtype == np.uint8
    assert np.array_equal(mask, gold[p + "mask"]) and np.array_equal(ind, gold[p + "ind"]) and not np.asarray(overflow).any()
    want, want64 = gold[p + "anno_box"], gold[p + "anno64"]
    exact = [0, 1, 2, 8, 9] + ([] if c["norm"] else [3, 4, 5])
    assert np.array_equal(anno[..., exact].view(np.int32), want[..., exact].view(np.int32))
    trans = [6, 7] + ([3, 4, 5] if c["norm"] else [])
    assert gen.ulps(anno[..., trans], want64[..., trans]).max() <= 1
    assert gen.ulps(anno[..., trans], want[..., trans]).max() <= 2
    want_heat, _ = golden_heatmaps(case, gold)
    return sum(check_heatmap(g, w) for g, w in zip(heatmaps, want_heat))


@pytest.mark.parametrize("case", CASES)
def test_stored_digests_match_the_inputs(case, gold):
    assert gen.digest(case) == str(gold[case + ".inputs_sha256"])
    boxes, labels, offsets = gen.packed(case)
    assert boxes.dtype == np.float32 and boxes.shape[1] == 9 and labels.dtype == np.int64 and offsets.dtype == np.int32 and len(offsets) == gen.B + 1


@pytest.mark.parametrize("case", CASES)
def test_host_mirror_reproduces_the_reference(case, gold):
    c = gen.CASES[case]
    out = head_targets._targets_host(*gen.packed(case), list(c["classes"]), c["cfg"], norm_bbox=c["norm"])
    assert check_case(case, gold, *out) == 0
    heat, overflow = head_targets._targets_host(*gen.packed(case, tf=True), sum(c["classes"]), c["cfg"])
    assert check_heatmap(heat, golden_heatmaps(case, gold)[1]) == 0 and not overflow.any()


def test_cases_hold_what_they_are_for(gold):
    """The fixture's cases exercise the paths they name (on the reference's own outputs)."""
    m = gold["edges.mask"]                                        # task 1, sample 0: skipped boxes leave zero slots between live ones
    assert m[1, 0, :8].tolist() == [1, 1, 0, 0, 1, 0, 1, 0] and m[2].sum() == 0 and m[:, 1].sum() == 0
    assert gold["edges.ind"][1, 0, 1] == 7                        # the coordinate in (-1, 0): cell 0
    assert (golden_heatmaps("edges", gold)[0][1][0, 1] > 0).all()  # the 30 m box covers its whole plane
    t = gold["truncate.mask"]
    assert t.shape[2] == 6 and t[1, 0].all()
    labels = gen.inputs("truncate")["labels"][0]
    assert (labels == 1).sum() + (labels == 2).sum() == 9


def test_host_mirror_bound_overflow():
    c = gen.CASES["mixed"]
    boxes, labels, offsets = gen.packed("mixed")
    heatmaps, anno, ind, mask, overflow = head_targets._targets_host(boxes, labels, offsets, list(c["classes"]), c["cfg"], max_boxes_per_sample=12)
    assert overflow.tolist() == [0, 1]
    assert all(not h[1].any() for h in heatmaps) and not np.stack(mask)[:, 1].any() and np.stack(mask)[:, 0].any()


def test_argument_errors():
    c = gen.CASES["mixed"]
    boxes, labels, offsets = [torch.from_numpy(a) for a in gen.packed("mixed")]
    lists = ([boxes[:12], boxes[12:]], [labels[:12], labels[12:]])
    wide = dict(c["cfg"], grid_size=[128, 160, 1])
    for fn, classes in ((heads.centerhead_get_targets, [1, 2, 2]), (heads.transfusion_heatmap_targets, 5)):
        with pytest.raises(ValueError, match="row/column"):
            fn(*lists, classes, wide)
        with pytest.raises(ValueError, match="1024"):
            fn((boxes, labels, offsets), None, classes, c["cfg"], max_boxes_per_sample=1025)
        with pytest.raises(ValueError, match="max_boxes_per_sample"):
            fn((boxes, labels, offsets), None, classes, c["cfg"])
        with pytest.raises(RuntimeError, match="GPU tensors"):                       # no CPU path
            fn(*lists, classes, c["cfg"])
        with pytest.raises(RuntimeError, match="GPU tensors"):
            fn((boxes, labels, offsets), None, classes, c["cfg"], max_boxes_per_sample=16)
    with pytest.raises(ValueError, match="65 classes"):
        heads.centerhead_get_targets(*lists, [8] * 8 + [1], c["cfg"])
    with pytest.raises(ValueError, match="65 classes"):
        heads.transfusion_heatmap_targets(*lists, 65, c["cfg"])


def test_symbols_are_declared_and_bound():
    root = os.path.dirname(HERE)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "bevfusion_amd_ext.h")).read(), flags=re.S)
    ext = ctypes.CDLL(_capi.EXT_LIB_PATH)
    for name in ("bevamd_centerhead_targets", "bevamd_heatmap_targets"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _capi.ext_exported_names() and hasattr(ext, name)


def test_library_rejects_bad_arguments_before_any_gpu_work():
    lib = _capi.load()
    pc, vs, one = _capi.floats([-25.6, -25.6]), _capi.floats([0.4, 0.4]), _capi.ints([1])
    rc = lib.bevamd_centerhead_targets(None, None, None, 0, 9, 1, 1025, one, 1, 10, pc, vs, 8, 16, 0.1, 2, 1, None, None, None, None, None, None)
    assert rc == 4 and "max_boxes_per_sample" in _capi.last_error()
    rc = lib.bevamd_heatmap_targets(None, None, None, 0, 9, 1, 16, 65, pc, vs, 8, 16, 0.1, 2, None, None, None)
    assert rc == 4 and "65 classes" in _capi.last_error()
    rc = lib.bevamd_heatmap_targets(None, None, None, 0, 8, 1, 16, 5, pc, vs, 8, 16, 0.1, 2, None, None, None)
    assert rc == 1 and "7 or 9 columns" in _capi.last_error()
