"""CPU: the map segmentation metrics (bevfusion_amd/seg_head.py) without a GPU: the host path against
tests/golden/seg_head_ref.npz exactly, and the argument checks of the C entry point.  tests/test_gpu_seg_head.py imports `gen` and
`gold` from here."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi, heads, seg_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "seg_head_ref.npz")

_spec = importlib.util.spec_from_file_location("make_seg_head_golden", os.path.join(ROOT, "tests", "golden", "make_seg_head_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLDEN))
    assert str(g["inputs_sha256"]) == gen.digest(), "the seeded inputs changed: regenerate the golden"
    return g


def check_metrics(metrics, gold):
    assert list(metrics) == [str(k) for k in gold["counts.metric_names"]]
    assert np.array_equal(np.array([metrics[k] for k in metrics], np.float64), gold["counts.metric_values"])


def test_host_counts_and_metrics_are_the_reference(gold):
    pred, label = gen.counts_inputs()
    p, l = torch.from_numpy(pred), torch.from_numpy(label)
    for lab in (l, l.to(torch.uint8), l.float(), l.long() * 3):
        counts = heads.seg_iou_counts(p, lab)
        assert counts.dtype == torch.int64 and np.array_equal(counts.numpy(), gold["counts.counts"])
    assert np.array_equal(heads.seg_iou_counts(p, l, [0.5]).numpy(), gold["counts.counts"][:, 3:4])
    results = [dict(masks_bev=p[s], gt_masks_bev=l[s]) for s in range(p.shape[0])]
    check_metrics(heads.evaluate_map(results, list(gen.MAP_CLASSES)), gold)


def test_the_case_has_predictions_on_every_threshold(gold):
    """`>=` against `>` shows in the counts: 30 predictions sit exactly on each of the seven thresholds."""
    pred, label = gen.counts_inputs()
    want = gold["counts.counts"]
    assert want.shape == (6, 7, 3) and tuple(seg_head.MAP_THRESHOLDS) == gen.THRESHOLDS
    for i, t in enumerate(gen.THRESHOLDS):
        on = pred == np.float32(t)
        assert on.sum() >= 30
        strict = np.stack([((pred > np.float32(t)) & label).sum(axis=(0, 2, 3)), ((pred > np.float32(t)) & ~label).sum(axis=(0, 2, 3))], 1)
        assert (want[:, i, :2] - strict).sum() == on.sum()
    assert np.array_equal(want[..., 0] + want[..., 2], np.broadcast_to(label.sum(axis=(0, 2, 3))[:, None], (6, 7)))


def test_wrapper_rejects_bad_arguments():
    p, l = torch.zeros(2, 3, 5), torch.zeros(2, 3, 5, dtype=torch.bool)
    with pytest.raises(ValueError, match="thresholds"):
        heads.seg_iou_counts(p, l, [0.5] * 17)
    with pytest.raises(ValueError, match="thresholds"):
        heads.seg_iou_counts(p, l, [])
    with pytest.raises(ValueError, match="shapes"):
        heads.seg_iou_counts(p, l[:, :2])


def test_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = _capi.load()
    host = np.zeros(64, np.float64)
    buf = host.ctypes.data                                   # a non-null host address: a rejected call never dereferences it
    counts = lambda samples, hw, n, dt=3, classes=6, pred=buf: lib.bevamd_seg_iou_counts(pred, buf, dt, samples, classes, hw, buf, n, buf, None)  # noqa: E731
    assert counts(3, 100, 17) == 1 and "thresholds" in _capi.last_error()
    assert counts(3, 100, 0) == 1 and "thresholds" in _capi.last_error()
    assert counts(0, 100, 7) == 1 and "bad sizes" in _capi.last_error()
    assert counts(3, 0, 7) == 1 and "bad sizes" in _capi.last_error()
    assert counts(3, 100, 7, classes=0) == 1 and counts(3, 100, 7, classes=1025) == 1
    assert counts(3, 1 << 36, 7) == 1 and "bad sizes" in _capi.last_error()
    assert counts(3, 100, 7, pred=None) == 1 and "null" in _capi.last_error()
    assert counts(3, 100, 7, dt=1) == 4 and "label_dtype" in _capi.last_error()
