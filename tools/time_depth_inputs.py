"""Depth inputs of BaseDepthTransform with every option (csrc/vtransform.hip: zeroed bin planes + scatter + pixel pass), 8 frames at
256x704, D = 59, timed in ONE process, the four candidates alternating round by round:
  (a) the module's device path (bevamd_depth_inputs_batch_zero_ws),
  (b) a plain-torch restatement of the reference's loop (base.py:269-329: zeros, per sample, per camera boolean indexing) on the same GPU,
  (c) torch.zeros of the output shape alone,
  (d) the existing scalar raster on the same clouds (bevamd_depth_raster_batch_zero_ws).
Two workloads: one-hot + height_expand + features on radar-like clouds (8 x 1 500 x F = 18) and one-hot + features on LiDAR clouds
(8 x ~310 k x F = 5).  Expected relations: (a) < (b), and (a) <= (c) + (d) + the run-to-run spread of (c) in this run.
    tools/time_depth_inputs.py [out.json] [rounds]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bevfusion_amd import synth
from bevfusion_amd.vtransforms import BaseDepthTransform

OUT = sys.argv[1] if len(sys.argv) > 1 else None
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 12
B, N_CAM, D = 8, 6, 59
dev = torch.device("cuda:0")
cfg = dict(synth.CL_CONFIG, feature_size=(8, 22), dbound=(1.0, 60.0, 1.0))
iH, iW = cfg["image_size"]


def module(depth_input, expand, feats):
    vt = BaseDepthTransform(256, 80, cfg["image_size"], cfg["feature_size"], cfg["xbound"], cfg["ybound"], cfg["zbound"], cfg["dbound"],
                            depth_input=depth_input, height_expand=expand, add_depth_features=feats).to(dev)
    assert vt.D == D
    return vt


def calibration(seed):
    rng = np.random.default_rng(seed)
    rig = synth.camera_rig(N_CAM)
    aug = synth.training_augmentation(rng, B, N_CAM, cfg)
    c2l = np.tile(np.eye(4), (N_CAM, 1, 1))
    c2l[:, :3, :3], c2l[:, :3, 3] = rig["camera2lidar_rots"], rig["camera2lidar_trans"]
    K = np.tile(np.eye(4), (N_CAM, 1, 1))
    K[:, :3, :3] = rig["intrins"]
    l2i = np.tile((K @ np.linalg.inv(c2l))[None], (B, 1, 1, 1)).astype(np.float32)
    ia = np.tile(np.eye(4, dtype=np.float32), (B, N_CAM, 1, 1))
    ia[..., :3, :3], ia[..., :3, 3] = aug["post_rots"], aug["post_trans"]
    la = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    la[:, :3, :3], la[:, :3, 3] = aug["extra_rots"], aug["extra_trans"]
    return [torch.from_numpy(a).to(dev) for a in (l2i, ia, la)]


def reference_loop(points, l2i_all, ia_all, la_all, one_hot, expand, feats):
    """base.py:269-329 op for op on device tensors (the tool's own restatement; clones instead of overwriting its inputs)."""
    points = [p.clone() for p in points]
    if expand:
        for b in range(len(points)):
            rep = points[b].repeat_interleave(8, dim=0)
            rep[:, 2] = torch.arange(0.25, 2.25, 0.25, device=dev).repeat(points[b].shape[0])
            points[b] = rep
    ch = (D if one_hot else 1) + (points[0].shape[1] if feats else 0)
    depth = torch.zeros(len(points), N_CAM, ch, iH, iW, device=dev)
    for b in range(len(points)):
        cur = points[b][:, :3]
        ia, la, l2i = ia_all[b], la_all[b], l2i_all[b]
        cur -= la[:3, 3]
        cur = torch.inverse(la[:3, :3]).matmul(cur.transpose(1, 0))
        cur = l2i[:, :3, :3].matmul(cur)
        cur += l2i[:, :3, 3].reshape(-1, 3, 1)
        dist = cur[:, 2, :]
        cur[:, 2, :] = torch.clamp(cur[:, 2, :], 1e-5, 1e5)
        cur[:, :2, :] /= cur[:, 2:3, :]
        cur = ia[:, :3, :3].matmul(cur)
        cur += ia[:, :3, 3].reshape(-1, 3, 1)
        cur = cur[:, :2, :].transpose(1, 2)[..., [1, 0]]
        on_img = (cur[..., 0] < iH) & (cur[..., 0] >= 0) & (cur[..., 1] < iW) & (cur[..., 1] >= 0)
        for c in range(N_CAM):
            mc = cur[c, on_img[c]].long()
            md = dist[c, on_img[c]]
            if one_hot:
                depth[b, c, torch.clamp(md, max=D - 1).long(), mc[:, 0], mc[:, 1]] = 1.0
            else:
                depth[b, c, 0, mc[:, 0], mc[:, 1]] = md
            if feats:
                depth[b, c, -points[b].shape[-1]:, mc[:, 0], mc[:, 1]] = points[b][on_img[c]].transpose(0, 1)
    return depth


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b) * 1e3


def stats(v):
    v = sorted(v)
    return dict(median_us=round(v[len(v) // 2], 1), min_us=round(v[0], 1), max_us=round(v[-1], 1), spread_us=round(v[-1] - v[0], 1))


def workload(name, clouds, depth_input, expand, feats):
    l2i, ia, la = calibration(11)
    img = torch.zeros(B, N_CAM, 1, 1, 1, device=dev)
    new, old = module(depth_input, expand, feats), module("scalar", False, False)
    F = clouds[0].shape[1]
    shape = (B, N_CAM, (D if depth_input == "one-hot" else 1) + (F if feats else 0), iH, iW)
    cands = dict(
        a_new_path=lambda: new.depth_raster(img, clouds, l2i, ia, la),
        b_torch_loop=lambda: reference_loop(clouds, l2i, ia, la, depth_input == "one-hot", expand, feats),
        c_zeros_only=lambda: torch.zeros(shape, device=dev),
        d_scalar_raster=lambda: old.depth_raster(img, clouds, l2i, ia, la))
    with torch.no_grad():
        got, ref = cands["a_new_path"](), cands["b_torch_loop"]()
        # the torch loop's index_put is unordered on collisions: compare the planes no winner is involved in, count the rest
        nb = D if depth_input == "one-hot" else 0
        bins_equal = bool(torch.equal(got[:, :, :nb], ref[:, :, :nb]))
        differing = int((got != ref).sum())
        del got, ref
        times = {k: [] for k in cands}
        for k, fn in cands.items():     # warm-up: allocator, persistent map, code objects
            for _ in range(2):
                timed(fn)
        for _ in range(ROUNDS):
            for k, fn in cands.items():
                times[k].append(timed(fn))
    res = {k: stats(v) for k, v in times.items()}
    out_bytes = int(np.prod(shape)) * 4
    map_bytes = B * N_CAM * iH * iW * 8 * 2 if (feats or depth_input == "scalar") else 0      # the pixel pass reads and clears the map
    a, b, c, d = (res[k]["median_us"] for k in cands)
    res.update(workload=name, points_per_sample=int(clouds[0].shape[0]), num_features=F, output_shape=list(shape), output_bytes=out_bytes,
               map_bytes=map_bytes, new_path_GBps=round((out_bytes + map_bytes) / a / 1e3, 1), zeros_GBps=round(out_bytes / c / 1e3, 1),
               rounds=ROUNDS, bin_planes_equal_torch_loop=bins_equal, words_differing_from_torch_loop=differing,
               a_lt_b=bool(a < b), a_le_c_plus_d_plus_spread=bool(a <= c + d + res["c_zeros_only"]["spread_us"]),
               c_plus_d_plus_spread_us=round(c + d + res["c_zeros_only"]["spread_us"], 1))
    print(json.dumps(res), flush=True)
    return res


def main():
    lidar = [synth.lidar_points(seed=70 + b, sweeps=10) for b in range(2)]
    rng = np.random.default_rng(5)
    radar = [np.concatenate([lidar[b % 2][1500 * b: 1500 * (b + 1)], rng.standard_normal((1500, 13)).astype(np.float32)], 1) for b in range(B)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    results = [workload("radar-like one-hot + height_expand + features", [t(p) for p in radar], "one-hot", True, True),
               workload("lidar one-hot + features", [t(lidar[b % 2]) for b in range(B)], "one-hot", False, True)]
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), image=[iH, iW], frames=B, cameras=N_CAM, depth_bins=D, workloads=results),
                      fh, indent=1)


if __name__ == "__main__":
    main()
