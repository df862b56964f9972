"""CPU: the CenterHead end — registry, argument checks and the host-tensor formulation against tests/golden/centerhead_ref.npz (the
REFERENCE's get_bboxes / get_task_detections statements and CenterPointBBoxCoder exec'd single-threaded on CPU torch by
tests/golden/make_centerhead_golden.py; inputs are regenerated here from the seed and checked against the stored SHA-256).

Bars: selection order, labels, kept rows and counts exactly equal; the centre and velocity columns of the boxes bit-equal (the
same fp32 operations in the same order); every column within `column_bars`: 4 x the reference fp32 result's own error against the
fixture's float64 values, per column, with a floor of 2 ulp of the column's largest magnitude (torch's vectorised exp / atan2 /
sigmoid need not give the bits of the same function on a gathered subset)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi, heads
from bevfusion_amd.registry import BBOX_CODERS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "centerhead_ref.npz")

_spec = importlib.util.spec_from_file_location("make_centerhead_golden", os.path.join(HERE, "golden", "make_centerhead_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

NAMES = ["x", "y", "z", "dx", "dy", "dz", "yaw", "vx", "vy"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def column_bars(ref32, ref64):
    """Per column: 4 x the reference's own fp32-vs-float64 error, at least 2 ulp of the column's largest magnitude."""
    e_ref = np.abs(ref32.astype(np.float64) - ref64).reshape(-1, ref32.shape[-1]).max(0)
    floor = 2 * np.spacing(np.abs(ref32).reshape(-1, ref32.shape[-1]).max(0).astype(np.float32)).astype(np.float64)
    return np.maximum(4 * e_ref, floor)


def case_preds(case, gold, dev="cpu"):
    assert gen.sha(*gen.arrays(case)) == str(gold[case + ".inputs_sha256"]), "inputs do not rebuild the fixture's bytes"
    return [[{k: torch.from_numpy(v).to(dev) for k, v in p[0].items()}] for p in gen.preds(case)]


def make_coder(case, **over):
    return heads.CenterPointBBoxCoder(**dict(gen.coder_args(case), **over))


def get_bboxes(case, preds, sync=True, **cfg):
    return heads.centerhead_get_bboxes(preds, make_coder(case), dict(gen.test_cfg(case), **cfg), list(gen.CLASSES),
                                       norm_bbox=gen.CASES[case]["norm"], sync=sync)


def kept_rows(case, gold):
    counts = gold[case + ".counts"]
    return np.split(gold[case + ".rows"].astype(np.int64), np.cumsum(counts)[:-1])


def check_case(case, gold, out, record=None):
    """out: the sync=False dict (any device) against the fixture; returns the per-column errors."""
    boxes, scores = out["bboxes"].cpu().numpy(), out["scores"].cpu().numpy()
    ref, ref64 = gold[case + ".boxes"], gold[case + ".boxes64"]
    assert boxes.shape == ref.shape
    exact = [0, 1] + ([7, 8] if gen.CASES[case]["vel"] else [])
    assert same_bits(boxes[..., exact], ref[..., exact]), "centre / velocity columns differ from the reference's bits"
    bars = column_bars(ref, ref64)
    err = np.abs(boxes.astype(np.float64) - ref64).reshape(-1, ref.shape[-1]).max(0)
    s_bar = column_bars(gold[case + ".scores"][..., None], gold[case + ".scores64"][..., None])[0]
    s_err = float(np.abs(scores.astype(np.float64) - gold[case + ".scores64"]).max())
    for j in range(ref.shape[-1]):
        print(f"{case} {NAMES[j]}: observed {err[j]:.3e}  bar {bars[j]:.3e}")
        if record:
            record(f"centerhead_ends/{case}/{NAMES[j]}", err[j], bars[j])
    print(f"{case} score: observed {s_err:.3e}  bar {s_bar:.3e}")
    if record:
        record(f"centerhead_ends/{case}/score", s_err, s_bar)
    assert np.all(err <= bars) and s_err <= s_bar
    assert out["labels"].dtype == torch.int32 and np.array_equal(out["labels"].cpu().numpy(), gold[case + ".labels"])
    rows = kept_rows(case, gold)
    for i in range(len(rows)):
        assert np.array_equal(np.nonzero(out["keep"][i].cpu().numpy())[0], rows[i]), f"sample {i}: kept rows differ"
    assert out["counts"].dtype == torch.int32 and out["counts"].tolist() == [len(r) for r in rows]
    return rows


def check_sync(out, res, rows):
    """The sync=True list equals the sync=False rows under `keep`, row for row."""
    assert len(res) == len(rows)
    for i, r in enumerate(rows):
        r = torch.from_numpy(r).to(out["bboxes"].device)
        assert torch.equal(res[i]["bboxes"], out["bboxes"][i][r]) and torch.equal(res[i]["scores"], out["scores"][i][r])
        assert torch.equal(res[i]["labels"], out["labels"][i][r]) and res[i]["labels"].dtype == torch.int32
        assert torch.equal(out["bboxes"][i][out["keep"][i]], res[i]["bboxes"])


# ---- host formulation against the fixture ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(gen.CASES))
def test_host_get_bboxes_matches_the_reference(case, gold):
    """Over the cases: vel on / off, norm_bbox on / off, rotate / circle / a mixed per-task list, nms_scale absent / scalar /
    nested, 16 x 16 and 12 x 20 maps, K = 32 and 130, segments of 0, 1, 2, 65 and 130 live rows, pre_max_size and post_max_size."""
    preds = case_preds(case, gold)
    before = [{k: v.clone() for k, v in p[0].items()} for p in preds]
    out = get_bboxes(case, preds, sync=False)
    assert all(torch.equal(p[0][k], b[k]) for p, b in zip(preds, before) for k in b), "the inputs were modified"
    rows = check_case(case, gold, out)
    check_sync(out, get_bboxes(case, preds), rows)


def test_the_caps_bite(gold):
    for case, key, loose in (("premax_16_k32", "pre_max_size", 1000), ("postmax_16_k130", "post_max_size", 83)):
        preds = case_preds(case, gold)
        tight, free = get_bboxes(case, preds, sync=False), get_bboxes(case, preds, sync=False, **{key: loose})
        assert not torch.equal(tight["keep"], free["keep"]), key
    assert gold["postmax_16_k130.counts"].tolist() == [15, 15]           # 3 tasks x post_max_size 5, circle task included


def check_decode(reg, gold, dev="cpu"):
    """decode on its own: with `reg` it is what get_bboxes feeds (checked through the head's fixture), without it the + 0.5 path."""
    case, t = gen.DECODE_NOREG["case"], gen.DECODE_NOREG["task"]
    args = gen.decode_noreg_args(as_tensor=lambda a: torch.from_numpy(a).to(dev))
    assert gen.sha(*gen.decode_noreg_args()) == str(gold["decode_noreg.inputs_sha256"])
    coder = make_coder(case)
    if not reg:
        res = coder.decode(*args, reg=None, task_id=t)
        rows = np.split(gold["decode_noreg.rows"].astype(np.int64), np.cumsum(gold["decode_noreg.counts"])[:-1])
        ref, ref64 = gold["decode_noreg.boxes"], gold["decode_noreg.boxes64"]
        bars = column_bars(ref, ref64)
        for i, r in enumerate(rows):
            got = res[i]["bboxes"].cpu().numpy()
            assert same_bits(got[:, [0, 1, 2, 7, 8]], ref[i][r][:, [0, 1, 2, 7, 8]]) and np.all(np.abs(got - ref64[i][r]) <= bars)
            assert same_bits(res[i]["scores"].cpu().numpy(), gold["decode_noreg.scores"][i][r])
            assert res[i]["labels"].dtype == torch.float32 and np.array_equal(res[i]["labels"].cpu().numpy(), gold["decode_noreg.labels"][i][r])
        return
    d = gen.inputs(case)
    res = coder.decode(*args, reg=torch.from_numpy(d[f"reg{t}"]).to(dev), task_id=t)
    K = gen.CASES[case]["K"]
    ref, ref64 = gold[case + ".boxes"][:, t * K:(t + 1) * K], gold[case + ".boxes64"][:, t * K:(t + 1) * K]
    bars = column_bars(gold[case + ".boxes"], gold[case + ".boxes64"])
    for i in range(gen.B):
        got = res[i]["bboxes"].cpu().numpy()
        rows = np.array([int(np.nonzero((ref[i][:, :2].view(np.int32) == g[:2].view(np.int32)).all(1))[0][0]) for g in got], np.int64)
        assert np.all(np.diff(rows) > 0) and 0 < len(rows) < K             # a filtered subsequence in descending score
        want = ref64[i][rows].copy()
        want[:, 2] += want[:, 5] * 0.5                                      # the coder returns the gravity centre
        assert np.all(np.abs(got - want) <= bars + 1e-6 * (np.arange(9) == 2))
        assert np.array_equal(res[i]["labels"].cpu().numpy() + sum(gen.CLASSES[:t]), gold[case + ".labels"][i, t * K:(t + 1) * K][rows])


@pytest.mark.parametrize("reg", [True, False])
def test_host_coder_decode_matches_the_reference(reg, gold):
    check_decode(reg, gold)


def test_coder_builds_from_the_centerhead_config():
    cfg = dict(type="CenterPointBBoxCoder", pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
               max_num=500, score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9)
    coder = BBOX_CODERS.build(cfg)
    assert isinstance(coder, heads.CenterPointBBoxCoder) and coder.max_num == 500 and coder.code_size == 9 and coder.encode() is None
    assert "CenterPointBBoxCoder" in BBOX_CODERS and "TransFusionBBoxCoder" in BBOX_CODERS
    d = heads.CenterPointBBoxCoder([-51.2, -51.2], 8, [0.1, 0.1])
    assert (d.post_center_range, d.max_num, d.score_threshold, d.code_size) == (None, 100, None, 9)
    assert {"CenterPointBBoxCoder", "centerhead_get_bboxes", "rotate_nms_segments"} <= set(heads.__all__)


def tie_preds(dev="cpu"):
    """Two tasks on a 4 x 4 map whose logits come from two values: nearly every selected score ties.  Seeded: every call
    returns the same tensors."""
    rng = np.random.default_rng(3)
    preds = []
    for ct in (1, 2):
        p = dict(heatmap=torch.from_numpy(np.array([0.5, 1.5], np.float32)[rng.integers(0, 2, (2, ct, 4, 4))]),
                 reg=torch.from_numpy(rng.random((2, 2, 4, 4), dtype=np.float32)), height=torch.zeros(2, 1, 4, 4), dim=torch.zeros(2, 3, 4, 4),
                 rot=torch.tensor([0.6, 0.8]).view(1, 2, 1, 1).expand(2, 2, 4, 4).contiguous(), vel=torch.zeros(2, 2, 4, 4))
        preds.append([{k: v.to(dev) for k, v in p.items()}])
    return preds


TIE_CFG = dict(nms_type=["rotate", "circle"], min_radius=[1.0, 1e-6], post_max_size=83, pre_max_size=1000, nms_thr=0.99, score_threshold=0.1,
               post_center_limit_range=[])


def tie_coder():
    return heads.CenterPointBBoxCoder([-8.0, -8.0], 8, [0.5, 0.5], post_center_range=[-100.0] * 3 + [100.0] * 3, max_num=12, score_threshold=0.1)


def test_equal_scores_come_in_ascending_flat_index():
    preds = tie_preds()
    out = heads.centerhead_get_bboxes(preds, tie_coder(), TIE_CFG, [1, 2], sync=False)
    for t, ct in enumerate((1, 2)):
        flat = preds[t][0]["heatmap"].reshape(2, -1)
        for b in range(2):
            want = sorted(range(ct * 16), key=lambda i: (-float(flat[b, i]), i))[:12]
            got_scores = out["scores"][b, t * 12:(t + 1) * 12]
            assert torch.equal(got_scores, flat[b, want].sigmoid())
            cells = [i % 16 for i in want]
            x = (torch.tensor([c // 4 for c in cells]).float() + preds[t][0]["reg"][b, 0].reshape(-1)[cells]) * 8 * 0.5 + -8.0
            assert torch.equal(out["bboxes"][b, t * 12:(t + 1) * 12, 0], x)
            assert out["labels"][b, t * 12:(t + 1) * 12].tolist() == [i // 16 + t for i in want]
    assert len(np.unique(out["scores"].numpy())) == 2
    # two classes of one cell give the same box: with equal scores both NMS types keep the lower row
    p = tie_preds()
    p[1][0]["heatmap"][:] = -3.0
    p[1][0]["heatmap"][:, :, 1, 2] = 2.0
    for kind, kept in (("rotate", [0]), ("circle", [0])):
        cfg = dict(TIE_CFG, nms_type=["rotate", kind], min_radius=[1.0, 0.5])
        o = heads.centerhead_get_bboxes(p, tie_coder(), cfg, [1, 2], sync=False)
        assert np.nonzero(o["keep"][0, 12:].numpy())[0].tolist() == kept and o["labels"][0, 12:14].tolist() == [1, 2]


# ---- argument errors -------------------------------------------------------------------------------------------------------------
def test_wrapper_argument_errors():
    preds = tie_preds()
    with pytest.raises(RuntimeError, match="max_num"):
        heads.centerhead_get_bboxes(preds, heads.CenterPointBBoxCoder([-8, -8], 8, [0.5, 0.5], post_center_range=[-9] * 3 + [9] * 3, max_num=17),
                                    TIE_CFG, [1, 2])
    with pytest.raises(NotImplementedError):
        heads.centerhead_get_bboxes(preds, heads.CenterPointBBoxCoder([-8, -8], 8, [0.5, 0.5], max_num=8), TIE_CFG, [1, 2])
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        heads.CenterPointBBoxCoder([-8, -8], 8, [0.5, 0.5], max_num=8).decode(z(1, 1, 4, 4), z(1, 1, 4, 4), z(1, 1, 4, 4), z(1, 1, 4, 4), z(1, 3, 4, 4), None)
    with pytest.raises(RuntimeError, match="max_num"):
        heads.CenterPointBBoxCoder([-8, -8], 8, [0.5, 0.5], post_center_range=[-9] * 3 + [9] * 3, max_num=17).decode(
            z(1, 1, 4, 4), z(1, 1, 4, 4), z(1, 1, 4, 4), z(1, 1, 4, 4), z(1, 3, 4, 4), None)
    with pytest.raises(ValueError, match="nms_type"):
        heads.centerhead_get_bboxes(preds, tie_coder(), dict(TIE_CFG, nms_type="soft"), [1, 2])
    with pytest.raises(ValueError, match="nms_type"):
        heads.centerhead_get_bboxes(preds, tie_coder(), dict(TIE_CFG, nms_type=["rotate"]), [1, 2])
    with pytest.raises(RuntimeError, match="num_classes"):
        heads.centerhead_get_bboxes(preds, tie_coder(), TIE_CFG, [1, 3])
    bad = tie_preds()
    bad[1][0]["dim"] = z(2, 2, 4, 4)
    with pytest.raises(RuntimeError, match="dim must be float32"):
        heads.centerhead_get_bboxes(bad, tie_coder(), TIE_CFG, [1, 2])
    bad = tie_preds()
    bad[0][0]["rot"] = bad[0][0]["rot"].double()
    with pytest.raises(RuntimeError, match="rot must be float32"):
        heads.centerhead_get_bboxes(bad, tie_coder(), TIE_CFG, [1, 2])
    bad = tie_preds()
    del bad[1][0]["vel"]
    with pytest.raises(RuntimeError, match="vel"):
        heads.centerhead_get_bboxes(bad, tie_coder(), TIE_CFG, [1, 2])
    with pytest.raises(RuntimeError, match="boxes must be float32"):
        heads.rotate_nms_segments(z(2, 4, 5), None, 0.2)


def test_argument_errors_of_the_entry_points():
    """The C ABI checks its arguments before any GPU work."""
    lib = _capi.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ptrs, maps = (ctypes.c_void_p * 3)(p, p, p), (ctypes.c_void_p * 15)(*([p] * 15))
    cls, six = _capi.ints([1, 2, 2]), _capi.floats([0] * 6)
    assert lib.bevamd_centerpoint_select_workspace_bytes(8, 10, 128, 128) == 8 * 10 * 128 * 128 * 8
    assert lib.bevamd_centerpoint_select_workspace_bytes(0, 10, 128, 128) == 0
    sel = lambda *a: lib.bevamd_centerpoint_select(*a)   # noqa: E731
    for args, msg in (((ptrs, cls, 3, 2, 16, 16, 1025, 1), "max_num"), ((ptrs, cls, 3, 2, 16, 16, 257, 1), "max_num"),
                      ((ptrs, cls, 3, 2, 16, 16, 0, 1), "max_num"), ((ptrs, cls, 17, 2, 16, 16, 8, 1), "tasks"),
                      ((ptrs, cls, 3, 0, 16, 16, 8, 1), "bad sizes"), ((ptrs, _capi.ints([1, 9, 2]), 3, 2, 16, 16, 8, 1), "classes"),
                      ((None, cls, 3, 2, 16, 16, 8, 1), "host array"), ((ptrs, None, 3, 2, 16, 16, 8, 1), "host arrays")):
        assert sel(*args, p, p, p, 1 << 30, None) == 1 and msg in _capi.last_error(), args
    assert sel((ctypes.c_void_p * 3)(p, None, p), cls, 3, 2, 16, 16, 8, 1, p, p, p, 1 << 30, None) == 1 and "null heatmap" in _capi.last_error()
    assert sel(ptrs, cls, 3, 2, 16, 16, 8, 1, None, p, p, 1 << 30, None) == 1 and "null buffer" in _capi.last_error()
    assert sel(ptrs, cls, 3, 2, 16, 16, 8, 1, p, p, p, 16, None) == 2 and "workspace" in _capi.last_error()

    dec = lambda maps_, *a: lib.bevamd_centerpoint_decode(maps_, cls, None, 3, 2, 16, 16, 8, p, p, 1, 1, *a)   # noqa: E731
    assert dec(maps, None, six, 0.0, 0, 0.0, 0, None, p, p, p, p, None) == 1 and "coder" in _capi.last_error()
    assert dec(maps, six, None, 0.0, 0, 0.0, 0, None, p, p, p, p, None) == 1 and "post_center_range" in _capi.last_error()
    assert dec(None, six, six, 0.0, 0, 0.0, 0, None, p, p, p, p, None) == 1 and "map pointers" in _capi.last_error()
    assert dec(maps, six, six, 0.0, 0, 0.0, 0, None, p, None, p, p, None) == 1 and "null buffer" in _capi.last_error()
    holes = (ctypes.c_void_p * 15)(*([p] * 15))
    holes[7] = None
    assert dec(holes, six, six, 0.0, 0, 0.0, 0, None, p, p, p, p, None) == 1 and "task 1" in _capi.last_error()
    holes = (ctypes.c_void_p * 15)(*([p] * 15))
    holes[14] = None
    assert dec(holes, six, six, 0.0, 0, 0.0, 0, None, p, p, p, p, None) == 1 and "for every task or for none" in _capi.last_error()

    nms = lambda *a: lib.bevamd_rotate_nms_segments(*a)   # noqa: E731
    thr = _capi.floats([0.2])
    assert nms(p, 9, None, None, None, 4, 2000, 1, None, thr, None, None, 1000, 83, p, p, None) == 4 and "not supported" in _capi.last_error()
    assert nms(p, 5, None, None, None, 4, 32, 1, None, thr, None, None, 1000, 83, p, p, None) == 1 and "bad sizes" in _capi.last_error()
    assert nms(p, 9, None, None, None, 4, 32, 0, None, thr, None, None, 1000, 83, p, p, None) == 1 and "tasks" in _capi.last_error()
    assert nms(p, 9, None, None, None, 4, 32, 1, None, None, None, None, 1000, 83, p, p, None) == 1 and "task_thresh" in _capi.last_error()
    assert nms(p, 9, None, None, None, 4, 32, 1, None, thr, None, _capi.floats([1] * 8), 1000, 83, p, p, None) == 1 and "labels" in _capi.last_error()
    assert nms(None, 9, None, None, None, 4, 32, 1, None, thr, None, None, 1000, 83, p, p, None) == 1 and "null buffer" in _capi.last_error()
    assert nms(p, 9, None, None, None, 0, 32, 1, None, thr, None, None, 1000, 83, p, p, None) == 0      # no segments: nothing to do
