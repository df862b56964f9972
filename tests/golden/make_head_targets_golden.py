"""Writes tests/golden/head_targets_ref.npz: recorded outputs of the REFERENCE's head target code on seeded ground truth.

The reference's `core/utils/gaussian.py` is exec'd unmodified from where it lies.  `CenterHead.get_targets_single` is a method of a
class that cannot be constructed here: its statements (models/heads/bbox/centerpoint.py:432-582) are read from the file at run
time, dedented, exec'd, and bound to a namespace object carrying the attributes they read (train_cfg, class_names, task_heads,
norm_bbox).  The dense-heatmap statements of `TransFusionHead.get_targets_single` (transfusion.py:526-573) sit in the middle of a
method: they are read likewise and exec'd in a namespace holding the names they read (self, labels, gt_bboxes_3d, gt_labels_3d);
`heatmap` is taken from it afterwards.  All of it runs under inert `sys.modules` stubs on CPU torch with one thread.  `Boxes` is the
minimum of LiDARInstance3DBoxes the statements read: `.tensor` and `.gravity_center` (lidar_box3d.py:40-46).

Nothing of the reference's text is stored: only the SHA-256 of the seeded inputs and recorded results.  Heatmaps are stored as
their non-zero cells (flat index into the per-task [B, C_t, H, W] blocks laid end to end, and value).  `anno64` is `anno_box` with
the three transcendental column groups (log dims, sin, cos) replaced by a float64 evaluation rounded once to fp32; `main()` asserts
that the reference's own fp32 values lie within 1 ulp of it.  Inputs are NOT stored: `inputs()` regenerates them with numpy alone
(the tests import this file for it and check the stored digests).

Cases (B = 2, tasks of (1, 2, 2) classes, 16 x 16 maps of 3.2 m cells, min_radius 2, overlap 0.1 unless the case says otherwise):
mixed; truncate (max_objs 6, nine boxes of one task with interleaved classes); edges (0.8 m cells, so that the 30 m box has radius
16 and its window covers the whole map; cells 0 and 15, a coordinate in (-1, 0), centres at -1.5 and 16.2 cells, dx = 0, dy < 0,
labels of -1, an empty sample, a task with no box); overlap; radius_ties (32 x 32: boxes whose radius is within 4 fp32 ulp of an
integer, found by a seeded vectorised search and confirmed here with the reference's gaussian_radius); nonorm (norm_bbox=False; 9
columns: `main()` asserts that the reference's statements raise on 7-column boxes, `vx, vy = box[7:]`); config_shape (180 x 180, six
tasks, max_objs 500: the nuScenes CenterHead config).  The TransFusion variant of a case keeps the boxes flagged `tf`: all but the
out-of-map centres and the -1 labels of `edges`, where that code's negative slices are undefined.

    python tests/golden/make_head_targets_golden.py
"""
import functools
import hashlib
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "head_targets_ref.npz")
REF = "/root/reference/mmdet3d"

B = 2
SMALL = (1, 2, 2)
TRANS_COLS = (3, 4, 5, 6, 7)      # log dims (with norm_bbox), sin, cos


def _cfg(size, cell_voxel=0.4, max_objs=20, **over):
    half = size * 8 * cell_voxel / 2
    cfg = dict(grid_size=[size * 8, size * 8, 1], out_size_factor=8, voxel_size=[cell_voxel, cell_voxel, 8.0],
               point_cloud_range=[-half, -half, -5.0, half, half, 3.0], max_objs=max_objs, dense_reg=1, gaussian_overlap=0.1, min_radius=2)
    cfg.update(over)
    return cfg


CASES = {
    "mixed": dict(size=16, classes=SMALL, cfg=_cfg(16), norm=True, seed=901),
    "truncate": dict(size=16, classes=SMALL, cfg=_cfg(16, max_objs=3, dense_reg=2), norm=True, seed=902),
    "edges": dict(size=16, classes=SMALL, cfg=_cfg(16, cell_voxel=0.1), norm=True, seed=903),
    "overlap": dict(size=16, classes=SMALL, cfg=_cfg(16), norm=True, seed=904),
    "radius_ties": dict(size=32, classes=SMALL, cfg=_cfg(32, max_objs=40), norm=True, seed=905),
    "nonorm": dict(size=16, classes=SMALL, cfg=_cfg(16), norm=False, seed=906),
    "config_shape": dict(size=180, classes=(1, 2, 2, 1, 2, 2), cfg=_cfg(180, cell_voxel=0.075, max_objs=500), norm=True, seed=907),
}
MIN_TIES = 16


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def ulps(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _yaw(rng, n=None):
    """At least 0.05 rad away from every multiple of pi / 2."""
    return rng.integers(-2, 2, n) * (np.pi / 2) + rng.uniform(0.05, np.pi / 2 - 0.05, n)


def _box(cfg, u, v, dx, dy, rng):
    """One 9-column row with its centre at (u, v) CELLS of the feature map."""
    metres = cfg["voxel_size"][0] * cfg["out_size_factor"]
    pc = cfg["point_cloud_range"]
    return [pc[0] + u * metres, pc[1] + v * metres, rng.uniform(-3, 1), dx, dy, rng.uniform(0.5, 4.0), float(_yaw(rng)),
            rng.uniform(-5, 5), rng.uniform(-5, 5)]


def _random(cfg, size, n, rng, total, big=30.0):
    rows = [_box(cfg, rng.uniform(0.3, size - 0.3), rng.uniform(0.3, size - 0.3), rng.uniform(0.5, big), rng.uniform(0.5, big), rng)
            for _ in range(n)]
    return rows, list(rng.integers(0, total, n))


def _tie_sizes(cfg, rng, count):
    """(dx, dy) in metres whose fp32 gaussian radius is within 4 ulp of an integer: the radius is homogeneous of degree one in the
    sizes, so a float64 evaluation places a draw next to the integer and a relative jitter of 1e-5 spreads it over the ulps; the
    fp32 restatement below (the reference's operation order) keeps the hits.  main() confirms each with the reference's function."""
    f = np.float32
    n = 4000
    m = cfg["gaussian_overlap"]
    vs, osf = f(cfg["voxel_size"][0]), f(cfg["out_size_factor"])
    ratio, k = rng.uniform(0.4, 2.5, n), rng.integers(3, 9, n)
    b3, c3 = -2 * m * (ratio + 1), (m - 1) * ratio
    unit = (b3 + np.sqrt(b3 * b3 - 16 * m * c3)) / 2                     # radius of (h, w) = (ratio, 1) cells
    w_cells = k / unit * (1 + rng.uniform(-1e-5, 1e-5, n))
    dx = (w_cells * float(vs) * float(osf)).astype(f)
    dy = (w_cells * ratio * float(vs) * float(osf)).astype(f)
    w, h = dx / vs / osf, dy / vs / osf
    b3f = f(-2 * m) * (h + w)
    c3f = f(m - 1) * w * h
    r = (b3f + np.sqrt(b3f * b3f - f(4 * (4 * m)) * c3f)) / f(2)
    assert r.dtype == np.float32
    hit = np.nonzero(ulps(r, np.rint(r).astype(f)) <= 4)[0][:count]
    assert len(hit) == count, len(hit)
    return dx[hit], dy[hit]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(boxes: per sample [n, 9] fp32, labels: per sample [n] int64, tf: per sample [n] bool, the boxes of the TransFusion
    variant)."""
    c = CASES[case]
    cfg, size, total = c["cfg"], c["size"], sum(c["classes"])
    rng = np.random.default_rng(c["seed"])
    samples = []
    if case in ("mixed", "nonorm"):
        samples = [_random(cfg, size, n, rng, total) + (None,) for n in (12, 13)]
    elif case == "config_shape":
        samples = [_random(cfg, size, n, rng, total, big=12.0) + (None,) for n in (30, 31)]
    elif case == "truncate":
        rows, labels = _random(cfg, size, 13, rng, total)
        labels = [2, 0, 1, 2, 1, 3, 2, 1, 2, 1, 4, 2, 0]                   # task 1: nine boxes, classes interleaved; six slots
        samples = [(rows, labels, None), _random(cfg, size, 8, rng, total) + (None,)]
    elif case == "edges":
        spec = [  # (u, v, dx, dy, label, in the TransFusion variant)
            (0.5, 0.5, 2.0, 4.0, 0, True), (15.5, 15.3, 1.5, 3.0, 1, True), (-0.4, 7.2, 2.0, 2.0, 1, True), (-1.5, 5.0, 2.0, 2.0, 1, False),
            (5.0, 5.0, 2.0, 2.0, -1, False), (8.3, 9.1, 30.0, 30.0, 2, True), (16.2, 3.0, 2.0, 2.0, 2, False), (4.6, 11.7, 3.0, 1.0, 2, True),
            (7.0, 7.0, 0.0, 2.0, 1, True), (9.0, 3.0, 2.0, -1.0, 2, True), (12.0, 12.0, 4.0, 4.0, -1, False), (3.3, -0.7, 1.0, 1.0, 0, True),
        ]
        rows = [_box(cfg, u, v, dx, dy, rng) for u, v, dx, dy, _, _ in spec]
        samples = [(rows, [s[4] for s in spec], [s[5] for s in spec]), ([], [], [])]
    elif case == "overlap":
        spec = [(6.4, 6.6, 3.0, 3.0, 1), (6.7, 6.2, 30.0, 28.0, 1), (10.2, 4.5, 4.0, 4.0, 3), (10.8, 4.1, 20.0, 25.0, 4),
                (3.5, 10.5, 2.0, 2.0, 0), (5.5, 11.5, 2.0, 2.0, 0), (4.5, 13.5, 2.0, 2.0, 0), (6.1, 6.9, 15.0, 18.0, 2)]
        first = ([_box(cfg, u, v, dx, dy, rng) for u, v, dx, dy, _ in spec], [s[4] for s in spec], None)
        rows = [_box(cfg, rng.uniform(5, 11), rng.uniform(5, 11), rng.uniform(1, 40), rng.uniform(1, 40), rng) for _ in range(14)]
        samples = [first, (rows, list(rng.integers(0, 2, 14)), None)]
    elif case == "radius_ties":
        dx, dy = _tie_sizes(cfg, rng, 24)
        for s in range(B):
            rows = [_box(cfg, rng.uniform(0.3, size - 0.3), rng.uniform(0.3, size - 0.3), float(dx[i]), float(dy[i]), rng)
                    for i in range(s * 12, s * 12 + 12)]
            samples.append((rows, list(rng.integers(0, total, 12)), None))
    out = dict(boxes=[], labels=[], tf=[])
    for rows, labels, tf in samples:
        out["boxes"].append(np.asarray(rows, np.float32).reshape(-1, 9))
        out["labels"].append(np.asarray(labels, np.int64).reshape(-1))
        out["tf"].append(np.ones(len(labels), bool) if tf is None else np.asarray(tf, bool).reshape(-1))
    if case == "radius_ties":                                             # the fp32 rows carry the searched sizes bit for bit
        got = np.concatenate(out["boxes"])[:, 3:5]
        assert np.array_equal(got[:, 0], dx) and np.array_equal(got[:, 1], dy)
    return out


def packed(case, tf=False):
    """(boxes [M, 9] fp32, labels [M] int64, offsets [B + 1] int32) of the case (tf: of its TransFusion variant)."""
    d = inputs(case)
    keep = d["tf"] if tf else [np.ones(len(l), bool) for l in d["labels"]]
    boxes = np.concatenate([b[k] for b, k in zip(d["boxes"], keep)]).astype(np.float32).reshape(-1, 9)
    labels = np.concatenate([l[k] for l, k in zip(d["labels"], keep)]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum([int(k.sum()) for k in keep])]).astype(np.int32)
    return boxes, labels, offsets


def digest(case):
    return sha(*packed(case), *packed(case, tf=True))


def dense_heatmap(idx, val, count):
    flat = np.zeros(count, np.float32)
    flat[idx] = val
    return flat


def split_heatmaps(flat, classes, size):
    """The packed buffer -> per task [B, C_t, size, size]."""
    out, base = [], 0
    for c in classes:
        out.append(flat[base:base + B * c * size * size].reshape(B, c, size, size))
        base += B * c * size * size
    return out


# ---- the reference, exec'd under stubs -------------------------------------------------------------------------------------
def load_reference():
    import torch

    torch.set_num_threads(1)
    path = os.path.join(REF, "core/utils/gaussian.py")
    gauss = types.ModuleType("reference_gaussian")
    exec(compile(open(path).read(), path, "exec"), gauss.__dict__)

    def block(rel, first, last, sentinel):
        path = os.path.join(REF, rel)
        src = textwrap.dedent("\n".join(open(path).read().split("\n")[first - 1:last]))
        assert src.split("\n")[0].startswith(sentinel), (first, src.split("\n")[0])
        return compile("\n" * (first - 1) + src, path, "exec")

    stubs = {k: types.ModuleType(k) for k in ("mmcv", "mmdet", "mmdet3d")}
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        ns = dict(torch=torch, gaussian_radius=gauss.gaussian_radius, draw_heatmap_gaussian=gauss.draw_heatmap_gaussian)
        exec(block("models/heads/bbox/centerpoint.py", 432, 582, "def get_targets_single("), ns)
        dense = block("models/heads/bbox/transfusion.py", 526, 573, "# # compute dense heatmap targets")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    head = type("Head", (), dict(get_targets_single=ns["get_targets_single"]))

    def transfusion_heatmap(boxes, labels, num_classes, cfg):
        env = dict(torch=torch, gaussian_radius=gauss.gaussian_radius, draw_heatmap_gaussian=gauss.draw_heatmap_gaussian,
                   self=types.SimpleNamespace(train_cfg=cfg, num_classes=num_classes), labels=labels, gt_bboxes_3d=boxes,
                   gt_labels_3d=labels)
        exec(dense, env)
        return env["heatmap"]

    return gauss, head, transfusion_heatmap


class Boxes:
    """The minimum of LiDARInstance3DBoxes that the target statements read."""

    def __init__(self, tensor):
        self.tensor = tensor

    @property
    def gravity_center(self):
        import torch

        centre = torch.zeros_like(self.tensor[:, :3])
        centre[:, :2] = self.tensor[:, :2]
        centre[:, 2] = self.tensor[:, 2] + self.tensor[:, 5] * 0.5
        return centre


def record(case, gauss, head_cls, transfusion_heatmap, out):
    import torch

    c = CASES[case]
    cfg, size, classes = c["cfg"], c["size"], list(c["classes"])
    d = inputs(case)
    T, max_objs = len(classes), cfg["max_objs"] * cfg["dense_reg"]
    head = head_cls()
    head.train_cfg, head.norm_bbox, head.task_heads = cfg, c["norm"], [None] * T
    names, flag = [], 0
    for ct in classes:
        names.append([f"c{flag + i}" for i in range(ct)])
        flag += ct
    head.class_names = names
    per_sample = [head.get_targets_single(Boxes(torch.from_numpy(b)), torch.from_numpy(l)) for b, l in zip(d["boxes"], d["labels"])]
    heat = [np.stack([s[0][t].numpy() for s in per_sample]) for t in range(T)]
    anno = np.stack([np.stack([s[1][t].numpy() for s in per_sample]) for t in range(T)])
    ind = np.stack([np.stack([s[2][t].numpy() for s in per_sample]) for t in range(T)])
    mask = np.stack([np.stack([s[3][t].numpy() for s in per_sample]) for t in range(T)])
    assert anno.shape == (T, B, max_objs, 10) and anno.dtype == np.float32 and ind.dtype == np.int64 and mask.dtype == np.uint8
    assert all(h.shape == (B, ct, size, size) and h.dtype == np.float32 for h, ct in zip(heat, classes))

    # the transcendental columns from float64, rounded once; the reference's fp32 lies within 1 ulp
    anno64 = anno.copy()
    worst = 0
    for b in range(B):
        flag = 0
        for t, ct in enumerate(classes):
            order = np.concatenate([np.nonzero(d["labels"][b] == flag + k)[0] for k in range(ct)])[:max_objs]
            assert mask[t, b, len(order):].sum() == 0
            for k, i in enumerate(order):
                if not mask[t, b, k]:
                    continue
                box = d["boxes"][b][i].astype(np.float64)
                assert np.abs(np.mod(box[6], np.pi / 2) - np.pi / 4) <= np.pi / 4 - 0.05 + 1e-6, (case, box[6])
                want = np.concatenate([np.log(box[3:6]) if c["norm"] else box[3:6], [np.sin(box[6]), np.cos(box[6])]]).astype(np.float32)
                anno64[t, b, k, 3:8] = want
                worst = max(worst, int(ulps(anno[t, b, k, 3:8], want).max()))
            flag += ct
    assert worst <= 1, (case, worst)

    tf_boxes, tf_labels, tf_off = packed(case, tf=True)
    total = sum(classes)
    centre = (tf_boxes[:, :2].astype(np.float64) - np.array(cfg["point_cloud_range"][:2])) / cfg["voxel_size"][0] / cfg["out_size_factor"]
    assert ((centre > -1) & (centre < size)).all() and ((tf_labels >= 0) & (tf_labels < total)).all(), case
    tf_heat = np.stack([transfusion_heatmap(Boxes(torch.from_numpy(tf_boxes[tf_off[b]:tf_off[b + 1]])),
                                            torch.from_numpy(tf_labels[tf_off[b]:tf_off[b + 1]]), total, cfg).numpy() for b in range(B)])
    assert tf_heat.shape == (B, total, size, size) and tf_heat.dtype == np.float32

    if case == "radius_ties":
        near = 0
        for b in range(B):
            for box in d["boxes"][b]:
                w = torch.tensor(box[3]) / torch.tensor(cfg["voxel_size"])[0] / cfg["out_size_factor"]
                l = torch.tensor(box[4]) / torch.tensor(cfg["voxel_size"])[1] / cfg["out_size_factor"]
                r = gauss.gaussian_radius((l, w), min_overlap=cfg["gaussian_overlap"]).numpy()
                near += int(ulps(r, np.rint(r)) <= 4)
        assert near >= MIN_TIES, near
        print(f"  radius_ties: {near} boxes within 4 ulp of an integer radius")
    if case == "nonorm":
        try:
            head.get_targets_single(Boxes(torch.from_numpy(d["boxes"][0][:, :7].copy())), torch.from_numpy(d["labels"][0]))
            raise AssertionError("the reference accepted 7-column boxes: record that case")
        except ValueError:
            pass                                                              # vx, vy = box[7:]: nothing to unpack

    p = case + "."
    flat = np.concatenate([h.ravel() for h in heat])
    nz = np.nonzero(flat)[0]
    out[p + "inputs_sha256"] = np.array(digest(case))
    out[p + "heatmap_idx"], out[p + "heatmap_val"] = nz.astype(np.int32), flat[nz]
    out[p + "anno_box"], out[p + "anno64"] = anno, anno64
    out[p + "ind"], out[p + "mask"] = ind.astype(np.int32), mask
    tf_flat = tf_heat.ravel()
    nz_tf = np.nonzero(tf_flat)[0]
    out[p + "tf_heatmap_idx"], out[p + "tf_heatmap_val"] = nz_tf.astype(np.int32), tf_flat[nz_tf]
    print(f"  {case}: {int(mask.sum())} live slots of {sum(len(l) for l in d['labels'])} boxes, {len(nz)} + {len(nz_tf)} heatmap cells, "
          f"{int((flat == 1).sum())} peaks, transcendental columns within {worst} ulp of float64")


def main():
    gauss, head_cls, transfusion_heatmap = load_reference()
    out = {}
    for case in CASES:
        record(case, gauss, head_cls, transfusion_heatmap, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
