"""Writes tests/golden/head_ends_ref.npz: recorded outputs of the REFERENCE's TransFusion head ends on seeded inputs.

The reference's `transfusion_bbox_coder.py` and `box3d_nms.py` are exec'd unmodified from where they lie, under inert
`sys.modules` stubs (mmdet, mmdet3d.ops, numba with `jit` as the identity), on CPU torch with one thread.  `forward_single` and
`get_bboxes` are methods of a class that cannot be constructed here: their statements at transfusion.py:239-282, :290-295,
:322-325 and :724-838 are read from the file at run time, dedented and exec'd against a namespace object carrying the attributes
they read.  Nothing of the reference's text is stored: only the seeded inputs' digests and recorded results.  Inputs are NOT
stored: `selection_inputs()`, `decode_inputs()` and `nms_inputs()` regenerate them (the tests import this file for them and check
the stored SHA-256).

Every case is built so that the reference's own answer is well defined (asserted below): selection logits are distinct multiples
of 2^-10, more than K cells survive and consecutive scores among the first K + 1 are at least 4 ulp apart; decode scores are
distinct and 1e-3 away from the 0.1 threshold, heights 0.5 m inside the range; NMS scores are distinct and every pairwise squared
distance is 1e-3 away from the radius.

    python tests/golden/make_head_ends_golden.py
"""
import hashlib
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "head_ends_ref.npz")
REF = "/root/reference/mmdet3d"

SELECTION_CASES = {
    "sel_nus": dict(B=2, C=10, H=24, W=24, Cf=16, K=32, k=3, dataset="nuScenes", seed=301),
    "sel_waymo": dict(B=2, C=3, H=24, W=24, Cf=16, K=32, k=3, dataset="Waymo", seed=302),
    "sel_rect": dict(B=2, C=10, H=20, W=28, Cf=16, K=32, k=3, dataset="nuScenes", seed=303),
}
# the flagship config's coder (configs/nuscenes/det/transfusion/default.yaml with the 0.075 m voxels)
CODER = dict(pc_range=[-54.0, -54.0], out_size_factor=8, voxel_size=[0.075, 0.075],
             post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], code_size=10)
RADIUS = 0.175
DECODE_CASES = {
    f"dec_{'vel' if v else 'novel'}_{'thr' if t else 'nothr'}_{n or 'none'}": dict(B=2, K=32, C=10, vel=v, score_threshold=t, nms_type=n,
                                                                                 dataset="nuScenes", seed=400 + 4 * i)
    for i, (v, t, n) in enumerate((v, t, n) for v in (True, False) for t in (0.0, 0.1) for n in (None, "circle"))
}
NMS_CASES = {
    "nms1": dict(N=1, side=2.0, pms=83, seed=501),
    "nms2": dict(N=2, side=0.4, pms=83, seed=502),
    "nms65": dict(N=65, side=6.0, pms=83, seed=503),
    "nms300": dict(N=300, side=20.0, pms=83, seed=504),
    "nms300_cap": dict(N=300, side=20.0, pms=20, seed=505),
}
SEGMENTED = dict(cases=("nms65", "nms300_cap", "nms2"), thresh=(RADIUS, -1.0, RADIUS))   # the middle segment keeps every row


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def ulps(a, b):
    """Distance in units of the last place between fp32 arrays of one sign."""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def selection_inputs(case):
    """(logits [B, C, H, W], feat [B, Cf, H * W], bev_pos [1, H * W, 2]) fp32; logits of a sample: distinct multiples of 2^-10 in
    [-6, 6]."""
    c = SELECTION_CASES[case]
    rng = np.random.default_rng(c["seed"])
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    logits = np.stack([(rng.choice(12289, size=C * H * W, replace=False) - 6144) / 1024.0 for _ in range(B)])
    feat = rng.standard_normal((B, c["Cf"], H * W)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    bev_pos = np.stack([xs, ys], -1).reshape(1, H * W, 2).astype(np.float32)
    return logits.reshape(B, C, H, W).astype(np.float32), feat, bev_pos


def _decode_draw(c, rng):
    B, K, C = c["B"], c["K"], c["C"]
    d = dict(heatmap=rng.uniform(-3, 3, (B, C, K)), rot=rng.uniform(-1, 1, (B, 2, K)), dim=rng.uniform(-0.5, 1.2, (B, 3, K)),
             height=rng.uniform(-2, 2, (B, 1, K)), query_heatmap_score=rng.uniform(0.05, 1.0, (B, C, K)))
    labels = rng.choice(C, size=(B, K), p=[0.04] * 8 + [0.34, 0.34])          # mostly pedestrians and cones: the NMS tasks
    centre = rng.uniform(5, 175, (B, 2, K))
    for b in range(B):                                                        # clusters: neighbours inside and outside the radius
        for cls in (8, 9):
            rows = np.nonzero(labels[b] == cls)[0]
            anchors = rng.uniform(20, 160, (3, 2))
            centre[b][:, rows] = (anchors[rng.integers(0, 3, len(rows))] + rng.uniform(-0.9, 0.9, (len(rows), 2))).T
        out = rng.choice(K, size=5, replace=False)
        centre[b, 0, out[:3]] = rng.uniform(193, 200, 3)                      # x beyond +61.2 m
        centre[b, 1, out[3:]] = rng.uniform(-20, -13, 2)                      # y beyond -61.2 m
    d["center"] = centre
    if c["vel"]:
        d["vel"] = rng.uniform(-5, 5, (B, 2, K))
    return {k: v.astype(np.float32) for k, v in d.items()}, labels.astype(np.int64)


def _decode_well_defined(c, d, labels):
    """float64 check of the margins that make the reference's answer unambiguous."""
    B, K = labels.shape
    h = np.take_along_axis(d["heatmap"].astype(np.float64), labels[:, None, :], 1)[:, 0]
    q = np.take_along_axis(d["query_heatmap_score"].astype(np.float64), labels[:, None, :], 1)[:, 0]
    score = q / (1 + np.exp(-h))
    z = d["height"][:, 0].astype(np.float64) - np.exp(d["dim"][:, 2].astype(np.float64)) * 0.5
    xy = d["center"].astype(np.float64) * 8 * 0.075 - 54.0
    if np.abs(score - 0.1).min() < 1e-3 or np.abs(z).max() > 9.5 or np.abs(np.abs(xy) - 61.2).min() < 1e-2:
        return False
    sides = [0, 0]
    for b in range(B):
        if len(np.unique(score[b].astype(np.float32))) != K:
            return False
        for cls in (8, 9):
            rows = np.nonzero(labels[b] == cls)[0]
            p = xy[b][:, rows].T
            d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)[np.triu_indices(len(rows), 1)]
            if len(d2) and np.abs(d2 - RADIUS).min() < 1e-3:
                return False
            sides[0] += int((d2 < RADIUS).sum())
            sides[1] += int((d2 > RADIUS).sum())
    return min(sides) >= 4


def decode_inputs(case):
    """(preds dict of fp32 arrays: heatmap [B, C, K] logits, rot, dim, height, center (cells), query_heatmap_score, optional vel;
    query_labels [B, K] int64).  The first draw of the seeded stream that keeps every margin."""
    c = DECODE_CASES[case]
    rng = np.random.default_rng(c["seed"])
    for _ in range(200):
        d, labels = _decode_draw(c, rng)
        if _decode_well_defined(c, d, labels):
            return d, labels
    raise AssertionError(f"{case}: no well-defined draw")


def nms_inputs(case):
    """dets [N, 3] fp32 (x, y, score): distinct scores, every pairwise squared distance 1e-3 away from RADIUS."""
    c = NMS_CASES[case]
    rng = np.random.default_rng(c["seed"])
    for _ in range(400):
        dets = np.concatenate([rng.uniform(0, c["side"], (c["N"], 2)), rng.uniform(0.05, 1, (c["N"], 1))], 1).astype(np.float32)
        p = dets[:, :2].astype(np.float64)
        d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)[np.triu_indices(c["N"], 1)]
        if len(np.unique(dets[:, 2])) == c["N"] and (len(d2) == 0 or np.abs(d2 - RADIUS).min() >= 1e-3):
            return dets
    raise AssertionError(f"{case}: no well-defined draw")


def segmented_inputs():
    """(dets [N, 3], seg_offsets [4] int32, thresh [3] fp32) of the three NMS cases laid end to end."""
    parts = [nms_inputs(n) for n in SEGMENTED["cases"]]
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.int32)
    return np.concatenate(parts), off, np.asarray(SEGMENTED["thresh"], np.float32)


# ---- the reference, exec'd under stubs -------------------------------------------------------------------------------------
def load_reference():
    import torch

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    class _Coders:
        def register_module(self, *a, **k):
            return lambda cls: cls

    def jit(*a, **k):
        if a and callable(a[0]):
            return a[0]
        return lambda f: f

    stubs = {
        "mmdet": mod("mmdet"), "mmdet.core": mod("mmdet.core"),
        "mmdet.core.bbox": mod("mmdet.core.bbox", BaseBBoxCoder=object),
        "mmdet.core.bbox.builder": mod("mmdet.core.bbox.builder", BBOX_CODERS=_Coders()),
        "numba": mod("numba", jit=jit),
        "mmdet3d": mod("mmdet3d"), "mmdet3d.ops": mod("mmdet3d.ops"), "mmdet3d.ops.iou3d": mod("mmdet3d.ops.iou3d"),
        "mmdet3d.ops.iou3d.iou3d_utils": mod("mmdet3d.ops.iou3d.iou3d_utils", nms_gpu=None, nms_normal_gpu=None),
    }
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        mods = {}
        for key, rel in (("coder", "core/bbox/coders/transfusion_bbox_coder.py"), ("nms", "core/post_processing/box3d_nms.py")):
            path = os.path.join(REF, rel)
            m = types.ModuleType("reference_" + key)
            exec(compile(open(path).read(), path, "exec"), m.__dict__)
            mods[key] = m
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    torch.set_num_threads(1)
    path = os.path.join(REF, "models/heads/bbox/transfusion.py")
    lines = open(path).read().split("\n")

    def block(first, last, sentinel):
        src = textwrap.dedent("\n".join(lines[first - 1:last]))
        assert sentinel in src.split("\n")[0], (first, src.split("\n")[0])
        return compile("\n" * (first - 1) + src, path, "exec")

    blocks = dict(select=block(239, 282, "heatmap = dense_heatmap.detach().sigmoid()"), pos=block(290, 295, "query_pos = bev_pos.gather("),
                  qscore=block(322, 325, 'ret_dicts[0]["query_heatmap_score"] = heatmap.gather('),
                  bboxes=block(724, 838, 'batch_size = preds_dict[0]["heatmap"].shape[0]'))
    return mods["coder"], mods["nms"], blocks


def record_selection(case, blocks, out):
    import torch
    from torch.nn import functional as F

    c = SELECTION_CASES[case]
    logits, feat, pos = selection_inputs(case)
    B, K = c["B"], c["K"]
    ns = dict(torch=torch, F=F, dense_heatmap=torch.from_numpy(logits), batch_size=B, lidar_feat_flatten=torch.from_numpy(feat),
              bev_pos=torch.from_numpy(pos).repeat(B, 1, 1), ret_dicts=[{}],
              self=types.SimpleNamespace(nms_kernel_size=c["k"], num_proposals=K, num_classes=c["C"], test_cfg=dict(dataset=c["dataset"])))
    for name in ("select", "pos", "qscore"):
        exec(blocks[name], ns)
    flat = ns["heatmap"].reshape(B, -1).numpy()
    for b in range(B):                                    # well defined: > K survivors, the first K + 1 scores >= 4 ulp apart
        top = np.sort(flat[b])[::-1][:K + 1]
        assert (flat[b] > 0).sum() > K and ulps(top[:-1], top[1:]).min() >= 4, case
    p = case + "."
    out[p + "inputs_sha256"] = np.array(sha(logits, feat, pos))
    out[p + "top_class"] = ns["top_proposals_class"].numpy().astype(np.int16)
    out[p + "top_index"] = ns["top_proposals_index"].numpy().astype(np.int16)
    out[p + "top_score"] = np.take_along_axis(flat, ns["top_proposals"].numpy(), 1)
    out[p + "query_heatmap_score"] = ns["ret_dicts"][0]["query_heatmap_score"].numpy()
    out[p + "query_feat_sha256"] = np.array(sha(ns["query_feat"].numpy()))
    out[p + "query_pos_sha256"] = np.array(sha(ns["query_pos"].numpy()))
    assert np.array_equal(ns["self"].query_labels.numpy(), ns["top_proposals_class"].numpy())


def _rows_of(sub, full):
    """Row indices of `sub` (an ordered subsequence of the rows of `full`, bit-equal)."""
    rows, j = [], 0
    for r in sub:
        while not np.array_equal(full[j].view(np.int32), r.view(np.int32)):
            j += 1
        rows.append(j)
        j += 1
    return np.asarray(rows, np.int16)


def record_decode(case, ref_coder, ref_nms, blocks, out):
    import torch
    from torch.nn import functional as F

    c = DECODE_CASES[case]
    d, labels = decode_inputs(case)
    B, K = labels.shape

    def coder():
        return ref_coder.TransFusionBBoxCoder(score_threshold=c["score_threshold"], **CODER)

    def preds(dtype):
        return {k: torch.from_numpy(v).to(dtype).clone() for k, v in d.items()}   # decode overwrites center and dim

    def full(dtype):
        pd = preds(dtype)
        score = pd["heatmap"].sigmoid() * pd["query_heatmap_score"] * F.one_hot(torch.from_numpy(labels), num_classes=c["C"]).permute(0, 2, 1)
        res = coder().decode(score, pd["rot"], pd["dim"], pd["center"], pd["height"], pd.get("vel"), filter=False)
        return (np.stack([r["bboxes"].numpy() for r in res]), np.stack([r["scores"].numpy() for r in res]),
                np.stack([r["labels"].numpy() for r in res]))

    box32, score32, label32 = full(torch.float32)
    box64, score64, _ = full(torch.float64)
    ns = dict(torch=torch, F=F, circle_nms=ref_nms.circle_nms, xywhr2xyxyr=None, nms_gpu=None, metas=None, preds_dict=[preds(torch.float32)],
              self=types.SimpleNamespace(num_proposals=K, num_classes=c["C"], query_labels=torch.from_numpy(labels), bbox_coder=coder(),
                                         test_cfg=dict(dataset=c["dataset"], nms_type=c["nms_type"])))
    exec(blocks["bboxes"], ns)
    ret = ns["ret_layer"]
    rows = [_rows_of(r["bboxes"].numpy(), box32[i]) for i, r in enumerate(ret)]
    for i, r in enumerate(ret):
        assert np.array_equal(r["scores"].numpy(), score32[i][rows[i]]) and np.array_equal(r["labels"].numpy(), label32[i][rows[i]])
    p = case + "."
    out[p + "inputs_sha256"] = np.array(sha(*[d[k] for k in sorted(d)], labels))
    out[p + "boxes"], out[p + "scores"], out[p + "labels"] = box32, score32, label32.astype(np.int16)
    out[p + "boxes64"], out[p + "scores64"] = box64, score64
    out[p + "counts"] = np.asarray([len(r) for r in rows], np.int32)
    out[p + "rows"] = np.concatenate(rows)


def record_nms(ref_nms, out):
    kept = {}
    for case, c in NMS_CASES.items():
        dets = nms_inputs(case)
        kept[case] = np.asarray(ref_nms.circle_nms(dets, RADIUS, c["pms"]), np.int16)
        out[case + ".inputs_sha256"] = np.array(sha(dets))
        out[case + ".keep"] = kept[case]
    assert len(ref_nms.circle_nms(nms_inputs("nms300"), RADIUS, 10 ** 6)) > 83 > NMS_CASES["nms300_cap"]["pms"]
    assert len(kept["nms2"]) == 1 and 1 < len(kept["nms65"]) < 65
    dets, off, thr = segmented_inputs()
    out["segmented.inputs_sha256"] = np.array(sha(dets, off, thr))
    for s, name in enumerate(SEGMENTED["cases"]):        # transfusion.py:823-824: a non-positive radius keeps every row
        rows = kept[name] if thr[s] > 0 else np.arange(off[s + 1] - off[s], dtype=np.int16)
        out[f"segmented.keep{s}"] = np.sort(rows) + off[s]


def main():
    ref_coder, ref_nms, blocks = load_reference()
    out = {}
    for case in SELECTION_CASES:
        record_selection(case, blocks, out)
    for case in DECODE_CASES:
        record_decode(case, ref_coder, ref_nms, blocks, out)
    record_nms(ref_nms, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    for case in DECODE_CASES:
        print(f"  {case}: kept {out[case + '.counts'].tolist()} of {DECODE_CASES[case]['K']}")
    for case in NMS_CASES:
        print(f"  {case}: kept {len(out[case + '.keep'])} of {NMS_CASES[case]['N']}")


if __name__ == "__main__":
    main()
