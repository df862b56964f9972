"""Writes tests/golden/seg_head_ref.npz: recorded outputs of the REFERENCE's map metrics on seeded inputs.

The counting statements of `NuScenesDataset.evaluate_map` (datasets/nuscenes_dataset.py:498-530) belong to a class that cannot be
imported here: they are read from the file at run time, dedented, exec'd on CPU torch with one thread, and bound to a namespace
object carrying `map_classes`.  Nothing of the reference's text is stored: only the SHA-256 of the seeded inputs and the recorded
results (the [K, T, 3] tp / fp / fn counts, which `main()` asserts reproduce the reference's metrics, and the metrics dict as
names and values).  Inputs are NOT stored: `counts_inputs` regenerates them with numpy alone (the tests import this file for it and
check the stored digest).

The case: [3, 6, 37, 41] (hw 1517: odd, more than one workgroup per class), the reference's seven thresholds, 30 predictions
planted exactly on each threshold (`>=` against `>`), labels true with probability 0.4.

    python tests/golden/make_seg_head_golden.py
"""
import functools
import hashlib
import os
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "seg_head_ref.npz")
REF = "/root/reference/mmdet3d"

MAP_CLASSES = ("drivable_area", "ped_crossing", "walkway", "stop_line", "carpark_area", "divider")
THRESHOLDS = (0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65)
COUNTS_SHAPE = (3, 6, 37, 41)
COUNTS_SEED = 1301


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def counts_inputs():
    """(pred fp32 [S, K, H, W] with 30 values per threshold planted exactly on it, label bool)."""
    rng = np.random.default_rng(COUNTS_SEED)
    pred = rng.uniform(0, 1, COUNTS_SHAPE).astype(np.float32)
    thr = np.array(THRESHOLDS, np.float32)
    spots = rng.choice(pred.size, 30 * len(thr), replace=False)
    pred.reshape(-1)[spots] = np.repeat(thr, 30)
    label = rng.uniform(0, 1, COUNTS_SHAPE) < 0.4
    return pred, label


def digest():
    return sha(*counts_inputs())


def load_reference():
    import torch

    torch.set_num_threads(1)
    path = os.path.join(REF, "datasets/nuscenes_dataset.py")
    first, last = 498, 530
    src = textwrap.dedent("\n".join(open(path).read().split("\n")[first - 1:last]))
    assert src.split("\n")[0].startswith("def evaluate_map("), src.split("\n")[0]
    ns = dict(torch=torch)
    exec(compile("\n" * (first - 1) + src, path, "exec"), ns)
    return type("Dataset", (), dict(evaluate_map=ns["evaluate_map"]))


def record_counts(dataset, out):
    import torch

    pred, label = counts_inputs()
    thr = torch.tensor(THRESHOLDS)
    S, K = pred.shape[:2]
    hit = torch.from_numpy(pred).reshape(S, K, -1, 1) >= thr
    truth = torch.from_numpy(label).reshape(S, K, -1, 1)
    counts = torch.stack([(hit & truth).sum(dim=(0, 2)), (hit & ~truth).sum(dim=(0, 2)), (~hit & truth).sum(dim=(0, 2))], dim=-1).numpy()
    ds = dataset()
    ds.map_classes = list(MAP_CLASSES)
    metrics = ds.evaluate_map([dict(masks_bev=torch.from_numpy(pred[s]), gt_masks_bev=torch.from_numpy(label[s])) for s in range(S)])
    # the recorded counts reproduce the reference's metrics: they are the reference's tp / fp / fn
    tp, fp, fn = (torch.from_numpy(counts[..., i]).float() for i in range(3))
    ious = tp / (tp + fp + fn + 1e-7)
    assert all(metrics[f"map/{name}/iou@max"] == ious[k].max().item() for k, name in enumerate(MAP_CLASSES))
    assert all(metrics[f"map/{name}/iou@{t:.2f}"] == ious[k, i].item() for k, name in enumerate(MAP_CLASSES) for i, t in enumerate(THRESHOLDS))
    on_threshold = int(sum((pred == np.float32(t)).sum() for t in THRESHOLDS))
    assert on_threshold >= 30 * len(THRESHOLDS)
    out["counts.counts"] = counts.astype(np.int64)
    out["counts.metric_names"] = np.array(list(metrics))
    out["counts.metric_values"] = np.array([metrics[k] for k in metrics], np.float64)
    print(f"  counts: {on_threshold} predictions on a threshold, {len(metrics)} metrics, mean iou@max {metrics['map/mean/iou@max']:.4f}")


def main():
    dataset = load_reference()
    out = {"inputs_sha256": np.array(digest())}
    record_counts(dataset, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
