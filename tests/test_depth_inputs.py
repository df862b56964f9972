"""CPU: the depth INPUT of `BaseDepthTransform` with every option of the reference (base.py:266-329) — depth_input scalar | one-hot,
height_expand, add_depth_features, LiDAR-like and radar-like clouds — against tests/golden/depth_inputs_ref.npz, outputs of the
REFERENCE's own `BaseDepthTransform.forward` exec'd single-threaded on CPU torch by tests/golden/make_depth_inputs_golden.py.
Everything is compared on the raw bits.

The fixture keeps each reference output [B, N, Cd, iH, iW] (up to 666 MB dense) as
  * the SHA-256 of its bytes,
  * one-hot: the linear indices of the bin planes' ones (delta-coded),
  * scalar / features: the hit pixels (delta-coded), the (virtual) point index whose row the reference left there and, scalar, the
    depth values;
`dense_reference()` rebuilds the dense tensor from those and the seeded clouds and checks the digest, so every comparison below is
against the reference's bytes.  (Feature planes hold raw point rows: their values stored one by one would not fit a committed file.)

Two side effects of the reference are NOT reproduced, on purpose: it overwrites the caller's point tensors (`-=` on a view,
base.py:290) and replaces the list entries by the 8x expanded clouds (base.py:273).  Ours leaves both untouched (asserted here)."""
import hashlib
import os

import numpy as np
import pytest
import torch

import oracle
from bevfusion_amd import synth
from bevfusion_amd.vtransforms import BaseDepthTransform

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_inputs_ref.npz")
CFG = dict(synth.CL_CONFIG, feature_size=(8, 22), dbound=(1.0, 60.0, 1.0))      # D = 59
N_CAM, BATCH = 6, 2
# (name, depth_input, height_expand, add_depth_features)
MODES = (("scalar_feat", "scalar", False, True), ("onehot", "one-hot", False, False), ("onehot_feat", "one-hot", False, True),
         ("onehot_expand_feat", "one-hot", True, True))
CLOUDS = ("lidar", "radar")
CASES = [(cloud, mode) for cloud in CLOUDS for mode in MODES]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_cloud(cloud, seed):
    """LiDAR-like: 40 000 rows of the synthetic spinning LiDAR, F = 5.  Radar-like: 1 500 of its rows with 13 seeded random columns
    appended, F = 18 (the reference's radar rows are that wide)."""
    pts = synth.lidar_points(seed=seed, sweeps=2)
    if cloud == "lidar":
        return np.ascontiguousarray(pts[:40000])
    extra = np.random.default_rng(1000 + seed).standard_normal((1500, 13)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([pts[:1500], extra], 1))


def expand_heights(pts):
    """base.py:269-273: every row 8 times, z = 0.25 .. 2.00."""
    rows = np.repeat(pts, 8, axis=0)
    rows[:, 2] = np.tile(np.arange(1, 9, dtype=np.float32) * np.float32(0.25), pts.shape[0])
    return rows


def reference_rows(pts, la, expand):
    """The rows the reference's feature planes show: (expanded) cloud with the LiDAR-augmentation translation subtracted in place."""
    rows = expand_heights(pts) if expand else pts.copy()
    rows[:, :3] -= la[:3, 3].astype(np.float32)
    return rows


def restate(pts, l2i, ia, la, inv, image_size, depth_input, n_bins, expand, feats):
    """numpy restatement of one sample: winners, depths and projection from `oracle.depth_raster` (pinned to the reference by
    tests/test_oracle_vtransform.py) on the expanded cloud for the scalar and feature planes; an all-hits pass (every virtual point
    alone, camera by camera) for the bins -> [N, Cd, iH, iW]."""
    iH, iW = image_size
    cloud = expand_heights(pts) if expand else pts
    n_cam = l2i.shape[0]
    F = pts.shape[1]
    one_hot = depth_input == "one-hot"
    nb = n_bins if one_hot else 1
    out = np.zeros((n_cam, nb + (F if feats else 0), iH * iW), np.float32)
    depth, winner = oracle.depth_raster(cloud, l2i, ia, la, image_size, inv_lidar_aug_rot=inv)
    hit = winner.reshape(n_cam, -1) >= 0
    if not one_hot:
        out[:, 0] = depth.reshape(n_cam, -1)
    if feats:
        rows = reference_rows(pts, la, expand)
        for c in range(n_cam):
            out[c, nb:, hit[c]] = rows[winner.reshape(n_cam, -1)[c, hit[c]]]
    if one_hot:
        for c, p, d in all_hits(cloud, l2i, ia, la, inv, image_size):
            out[c, np.minimum(d, np.float32(n_bins - 1)).astype(np.int64), p] = 1.0
    return out.reshape(n_cam, -1, iH, iW)


def all_hits(cloud, l2i, ia, la, inv, image_size):
    """Every (camera, pixels, depths) the points of the cloud land on, from the oracle's projection alone: per camera, raster the
    cloud, take the winners (a winner's pixel and depth are its own), drop them and raster the rest again until nothing lands."""
    for c in range(l2i.shape[0]):
        left = np.arange(cloud.shape[0])
        while left.size:
            depth, winner = oracle.depth_raster(cloud[left], l2i[c:c + 1], ia[c:c + 1], la, image_size, inv_lidar_aug_rot=inv)
            w = winner.reshape(-1)
            p = np.flatnonzero(w >= 0)
            if not p.size:
                break
            yield c, p, depth.reshape(-1)[p]
            keep = np.ones(left.size, bool)
            keep[w[p]] = False
            left = left[keep]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def clouds_of(gold, cloud):
    pts = [make_cloud(cloud, int(s)) for s in gold["points_seed"]]
    for p, h in zip(pts, gold[f"{cloud}_points_sha256"]):
        assert sha(p) == str(h), "synthetic cloud drifted from the fixture"
    return pts


def dense_reference(gold, cloud, mode, pts):
    """Rebuild the reference's [B, N, Cd, iH, iW] output of one case from the fixture; the digest of the reference's bytes checks it."""
    name, depth_input, expand, feats = mode
    k = f"{cloud}_{name}_"
    shape = tuple(int(v) for v in gold[k + "shape"])
    B, N, Cd, iH, iW = shape
    P = iH * iW
    out = np.zeros((B, N, Cd, P), np.float32)
    nb = Cd - (pts[0].shape[1] if feats else 0)
    if depth_input == "one-hot":
        out.reshape(-1)[np.cumsum(gold[k + "bins_dlin"].astype(np.int64))] = 1.0
    if depth_input == "scalar" or feats:
        lin = np.cumsum(gold[k + "win_dlin"].astype(np.int64))        # over [B, N, P]
        row = gold[k + "win_row"].astype(np.int64)
        b, c, p = lin // (N * P), lin // P % N, lin % P
        if depth_input == "scalar":
            out[b, c, 0, p] = gold[k + "win_depth"]
        if feats:
            for s in range(B):
                m = b == s
                rows = reference_rows(pts[s], gold["la"][s], expand)
                out[s, c[m], nb:, p[m]] = rows[row[m]]
    out = out.reshape(shape)
    assert sha(out) == str(gold[k + "sha256"]), "fixture does not rebuild the reference's bytes"
    return out


def make_module(mode, use_points="lidar"):
    _, depth_input, expand, feats = mode

    class Capture(BaseDepthTransform):
        def get_cam_feats(self, img, depth, mats):
            self.cap_depth = depth
            return torch.zeros(1)

        def bev_pool(self, geom_feats, x):
            return None

    return Capture(256, 80, CFG["image_size"], CFG["feature_size"], CFG["xbound"], CFG["ybound"], CFG["zbound"], CFG["dbound"],
                   use_points=use_points, depth_input=depth_input, height_expand=expand, add_depth_features=feats)


def run_forward(vt, pts, gold, dev=None):
    """forward(img, points, radar, sensor2ego, lidar2ego, lidar2camera, lidar2image, cam_intrinsic, camera2lidar, img_aug_matrix,
    lidar_aug_matrix, metas) with the clouds in the slot `use_points` names; returns (captured depth, the tensors handed in)."""
    t = lambda a: torch.from_numpy(np.array(a, copy=True)) if dev is None else torch.from_numpy(np.array(a, copy=True)).to(dev)  # noqa: E731
    handed = [t(p) for p in pts]
    lst = list(handed)
    img = t(np.zeros((len(pts), N_CAM, 1, 1, 1), np.float32))
    lidar, radar = (None, lst) if vt.use_points == "radar" else (lst, None)
    vt.forward(img, lidar, radar, t(gold["c2l"]), t(gold["c2l"]), None, t(gold["l2i"]), t(gold["K"]), t(gold["c2l"]), t(gold["ia"]),
               t(gold["la"]), None)
    assert len(lst) == len(handed) and all(a is b for a, b in zip(lst, handed)), "the caller's list was changed"
    for a, p in zip(handed, pts):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), p.view(np.uint32)), "the caller's points were changed"
    return vt.cap_depth


@pytest.mark.parametrize("cloud,mode", CASES, ids=[f"{c}-{m[0]}" for c, m in CASES])
def test_host_forward_equals_the_reference(gold, cloud, mode):
    pts = clouds_of(gold, cloud)
    ref = dense_reference(gold, cloud, mode, pts)
    vt = make_module(mode, use_points="radar" if cloud == "radar" else "lidar")
    assert vt.D == 59
    got = run_forward(vt, pts, gold).numpy()
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert int((ref != 0).sum()) > 1000


@pytest.mark.parametrize("cloud,mode", CASES, ids=[f"{c}-{m[0]}" for c, m in CASES])
def test_numpy_restatement_equals_the_reference(gold, cloud, mode):
    pts = clouds_of(gold, cloud)
    ref = dense_reference(gold, cloud, mode, pts)
    _, depth_input, expand, feats = mode
    for b, p in enumerate(pts):
        got = restate(p, gold["l2i"][b], gold["ia"][b], gold["la"][b], gold["inv_lidar_aug_rot"][b], CFG["image_size"], depth_input, 59,
                      expand, feats)
        assert np.array_equal(got.view(np.uint32), ref[b].view(np.uint32)), b


def test_every_option_combination_runs_on_host_tensors(gold):
    """No combination of the four options raises any more; channel counts follow base.py:276-278."""
    pts = [make_cloud("radar", int(s))[:200] for s in gold["points_seed"]]
    for depth_input in ("scalar", "one-hot"):
        for expand in (False, True):
            for feats in (False, True):
                for use_points in ("lidar", "radar"):
                    vt = make_module(("", depth_input, expand, feats), use_points=use_points)
                    d = run_forward(vt, pts, gold)
                    assert d.shape == (BATCH, N_CAM, (59 if depth_input == "one-hot" else 1) + (18 if feats else 0), 256, 704)


def test_arguments_are_validated_before_any_gpu_work():
    import ctypes

    from bevfusion_amd import _capi

    lib = _capi.load()
    one = (ctypes.c_int * 1)(1 << 29)
    ptrs = (ctypes.c_void_p * 1)(8)
    z = ctypes.c_void_p(8)
    assert lib.bevamd_depth_inputs_batch(ptrs, one, 1, 5, z, z, 3, z, z, 6, 8, 8, 2, 59, 0, 0, z, z, 1 << 30, None) == 1
    assert "depth_mode" in _capi.last_error()
    assert lib.bevamd_depth_inputs_batch(ptrs, one, 1, 5, z, z, 3, z, z, 6, 8, 8, 1, 0, 0, 0, z, z, 1 << 30, None) == 1
    assert "num_bins" in _capi.last_error()
    assert lib.bevamd_depth_inputs_batch(ptrs, one, 1, 5, z, z, 3, z, z, 6, 8, 8, 1, 59, 1, 0, z, z, 1 << 30, None) == 1
    assert "height_expand" in _capi.last_error()
    assert lib.bevamd_depth_inputs_batch(ptrs, one, 1, 5, z, z, 3, z, z, 6, 8, 8, 0, 0, 0, 0, z, None, 0, None) == 2      # no map
    assert lib.bevamd_depth_inputs_channels(1, 59, 18, 1) == 77 and lib.bevamd_depth_inputs_channels(0, 0, 5, 0) == 1
    assert lib.bevamd_depth_inputs_channels(3, 59, 18, 1) == 0
