"""Generates tests/golden/depth_inputs_ref.npz by running the REFERENCE's own `BaseDepthTransform.forward`
(`/root/reference/mmdet3d/models/vtransforms/base.py:238-361`, exec'd unmodified under the stubs of make_vtransform_golden.py)
on CPU torch, single-threaded (sequential `index_put`: the last point in input order wins a pixel), on COPIES of the inputs —
the reference overwrites the point tensors it is given and replaces the list entries by the 8x expanded clouds.

Cases: dbound (1, 60, 1) (D = 59), 256x704, 6 cameras, B = 2, the augmented matrices of `matrices()`;
  {scalar + features, one-hot, one-hot + features, one-hot + height_expand + features}
  x {LiDAR-like cloud, 40 000 rows, F = 5; radar-like cloud, 1 500 rows, F = 18 (13 seeded random columns appended)}.

Per case and cloud the generator asserts that the reference's SCALAR-mode depth equals `oracle.depth_raster` bit for bit on the same
(expanded) cloud: MKL's sgemm leaves the k-ascending FMA chain at some small n, which is a property of that library and not of the
reference's code; a cloud that trips it would not be a fixture the kernels can be pinned to.

Stored per case (see tests/test_depth_inputs.py::dense_reference, which this file uses to prove that the pieces rebuild the
reference's bytes before it writes them): SHA-256 of the dense output; one-hot: delta-coded linear indices of the ones; scalar /
features: delta-coded hit pixels, the virtual point index whose row the reference wrote there, the scalar depths.  The raw feature
values are rows of the seeded clouds and are not stored a second time.

    python tests/golden/make_depth_inputs_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
import test_depth_inputs as T  # noqa: E402
from make_vtransform_golden import load_reference_base, matrices  # noqa: E402

SEEDS = (31, 32)


def run_reference(ref, pts, m, depth_input, expand, feats):
    """-> (dense depth [B, N, Cd, iH, iW] numpy, inverses of lidar_aug[:3, :3] as the reference's calls returned them)."""
    class Capture(ref.BaseDepthTransform):
        def get_cam_feats(self, img, depth, mats):
            self.cap_depth = depth
            return torch.zeros(1)

        def bev_pool(self, geom_feats, x):
            return None

    cfg = T.CFG
    vt = Capture(256, 80, cfg["image_size"], cfg["feature_size"], cfg["xbound"], cfg["ybound"], cfg["zbound"], cfg["dbound"],
                 depth_input=depth_input, height_expand=expand, add_depth_features=feats)
    assert vt.D == 59
    t = lambda a: torch.from_numpy(a.copy())  # noqa: E731
    mats4 = {k: t(v) for k, v in m.items()}
    calls = []
    real_inverse = torch.inverse

    def recording_inverse(x):   # row-major result, recorded: see make_vtransform_golden.py
        r = real_inverse(x).contiguous()
        calls.append(r.clone())
        return r

    torch.inverse = recording_inverse
    try:
        vt.forward(torch.zeros(len(pts), T.N_CAM, 1, 1, 1), [t(p) for p in pts], None, mats4["c2l"], mats4["c2l"], None, mats4["l2i"],
                   mats4["K"], mats4["c2l"], mats4["ia"], mats4["la"], None)
    finally:
        torch.inverse = real_inverse
    return vt.cap_depth.numpy(), torch.stack(calls[: len(pts)]).numpy()


def delta(lin):
    d = np.diff(lin, prepend=0)
    assert (d >= 0).all() and d.max() < 2 ** 32
    return d.astype(np.uint32)


def main():
    torch.set_num_threads(1)
    ref = load_reference_base()
    m = matrices(T.N_CAM, T.BATCH, seed=7)
    fix = {k: m[k] for k in ("c2l", "K", "ia", "la", "l2i")}
    fix["points_seed"] = np.array(SEEDS)
    iH, iW = T.CFG["image_size"]
    P = iH * iW
    for cloud in T.CLOUDS:
        pts = [T.make_cloud(cloud, s) for s in SEEDS]
        fix[f"{cloud}_points_sha256"] = np.array([T.sha(p) for p in pts])
        winners = {}
        for expand in (False, True):
            # the condition that keeps the fixture on the arithmetic the kernels reproduce
            d, inv = run_reference(ref, pts, m, "scalar", expand, False)
            if "inv_lidar_aug_rot" in fix:
                assert np.array_equal(fix["inv_lidar_aug_rot"], inv)
            fix["inv_lidar_aug_rot"] = inv
            win = []
            for b, p in enumerate(pts):
                od, w = oracle.depth_raster(T.expand_heights(p) if expand else p, m["l2i"][b], m["ia"][b], m["la"][b], (iH, iW),
                                            inv_lidar_aug_rot=inv[b])
                assert np.array_equal(od.view(np.uint32), d[b].view(np.uint32)), (cloud, expand, b)
                win.append(w.reshape(-1))
            winners[expand] = np.concatenate(win)                       # [B * N * P]
        for mode in T.MODES:
            name, depth_input, expand, feats = mode
            d, inv = run_reference(ref, pts, m, depth_input, expand, feats)
            assert np.array_equal(inv, fix["inv_lidar_aug_rot"])
            k = f"{cloud}_{name}_"
            fix[k + "shape"] = np.array(d.shape)
            fix[k + "sha256"] = np.array(T.sha(d))
            F = pts[0].shape[1]
            nb = d.shape[2] - (F if feats else 0)
            if depth_input == "one-hot":
                bins = d[:, :, :nb]
                lin = np.flatnonzero(bins.reshape(-1))
                assert (bins.reshape(-1)[lin] == 1.0).all()
                b_, c_, r_ = np.unravel_index(lin, (d.shape[0], d.shape[1], nb * P))
                fix[k + "bins_dlin"] = delta((b_ * d.shape[1] + c_) * d.shape[2] * P + r_)      # index into the full [B, N, Cd, P]
            if depth_input == "scalar" or feats:
                lin = np.flatnonzero(winners[expand] >= 0)
                fix[k + "win_dlin"] = delta(lin)
                fix[k + "win_row"] = winners[expand][lin].astype(np.int32)
                if depth_input == "scalar":
                    fix[k + "win_depth"] = d[:, :, 0].reshape(-1)[lin]
            nnz = int((d != 0).sum())
            rebuilt = T.dense_reference(fix, cloud, mode, pts)           # asserts the digest
            assert np.array_equal(rebuilt.view(np.uint32), d.view(np.uint32))
            print(f"{cloud:5s} {name:20s} shape {d.shape} non-zeros {nnz} ({nnz // d.shape[0]} per sample)", flush=True)
    path = os.path.join(HERE, "depth_inputs_ref.npz")
    np.savez_compressed(path, **fix)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
