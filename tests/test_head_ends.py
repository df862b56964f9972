"""CPU: the TransFusion head ends — C ABI argument checks, registry, coder round trip and the host-tensor formulation against
tests/golden/head_ends_ref.npz (the REFERENCE's forward_single / get_bboxes statements, TransFusionBBoxCoder and circle_nms exec'd
single-threaded on CPU torch by tests/golden/make_head_ends_golden.py; inputs are regenerated here from the seed and checked
against the stored SHA-256).

Bars: indices, classes, labels and keep sets are exactly equal; scores and boxes are bit-equal in every column (the same torch ops
in the same order on the same CPU)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi, heads
from bevfusion_amd.registry import BBOX_CODERS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "head_ends_ref.npz")

_spec = importlib.util.spec_from_file_location("make_head_ends_golden", os.path.join(HERE, "golden", "make_head_ends_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def selection_case(case, gold, dev="cpu"):
    logits, feat, pos = gen.selection_inputs(case)
    assert gen.sha(logits, feat, pos) == str(gold[case + ".inputs_sha256"]), "inputs do not rebuild the fixture's bytes"
    return [torch.from_numpy(a).to(dev) for a in (logits, feat, pos)]


def select(case, tensors, **over):
    c = dict(gen.SELECTION_CASES[case], **over)
    return heads.transfusion_select_proposals(*tensors, num_proposals=c["K"], nms_kernel_size=c["k"], dataset=c["dataset"])


def make_coder(score_threshold=0.0):
    return heads.TransFusionBBoxCoder(score_threshold=score_threshold, **gen.CODER)


def decode_case(case, gold, dev="cpu"):
    d, labels = gen.decode_inputs(case)
    assert gen.sha(*[d[k] for k in sorted(d)], labels) == str(gold[case + ".inputs_sha256"]), "inputs do not rebuild the fixture's bytes"
    return {k: torch.from_numpy(v).to(dev) for k, v in d.items()}, torch.from_numpy(labels).to(dev)


def get_bboxes(case, preds, labels, sync=True):
    c = gen.DECODE_CASES[case]
    return heads.transfusion_get_bboxes(preds, labels, make_coder(c["score_threshold"]), dict(dataset=c["dataset"], nms_type=c["nms_type"]),
                                        c["K"], c["C"], sync=sync)


def kept_rows(case, gold):
    counts = gold[case + ".counts"]
    return np.split(gold[case + ".rows"].astype(np.int64), np.cumsum(counts)[:-1])


def nms_case(case, gold):
    dets = gen.nms_inputs(case)
    assert gen.sha(dets) == str(gold[case + ".inputs_sha256"])
    return dets


# ---- host formulation against the fixture ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(gen.SELECTION_CASES))
def test_host_selection_matches_the_reference(case, gold):
    tensors = selection_case(case, gold)
    before = tensors[0].clone()
    sel = select(case, tensors)
    assert torch.equal(tensors[0], before)
    assert np.array_equal(sel.top_proposals_class.numpy(), gold[case + ".top_class"])
    assert np.array_equal(sel.top_proposals_index.numpy(), gold[case + ".top_index"])
    assert sel.top_proposals_class.dtype == sel.top_proposals_index.dtype == torch.int64
    assert same_bits(sel.top_proposals_score.numpy(), gold[case + ".top_score"])
    assert same_bits(sel.query_heatmap_score.numpy(), gold[case + ".query_heatmap_score"])
    assert gen.sha(sel.query_feat.numpy()) == str(gold[case + ".query_feat_sha256"])
    assert gen.sha(sel.query_pos.numpy()) == str(gold[case + ".query_pos_sha256"])


def test_host_selection_is_a_stable_sort():
    """Equal scores come in ascending flat index, and zeros fill the list when fewer than K cells survive."""
    logits = torch.full((1, 10, 6, 6), -2.0)
    logits[0, 3, 2, 2] = logits[0, 1, 3, 3] = 1.0          # two equal peaks: class 1 has the lower flat index
    sel = heads.transfusion_select_proposals(logits, torch.zeros(1, 4, 36), torch.zeros(1, 36, 2), 8, 3, "nuScenes")
    flat = (sel.top_proposals_class * 36 + sel.top_proposals_index)[0].tolist()
    # behind the two peaks every interior cell of a flat plane ties with its own window: class 0's come first
    assert flat[:2] == [1 * 36 + 21, 3 * 36 + 14] and flat[2:] == [7, 8, 9, 10, 13, 14]
    assert sel.top_proposals_score[0].tolist() == [float(torch.tensor(1.0).sigmoid())] * 2 + [float(torch.tensor(-2.0).sigmoid())] * 6
    logits = -torch.arange(27.0).view(1, 3, 3, 3) / 10          # a ramp: no centre cell is its plane's maximum ...
    logits[0, 0, 1, 1], logits[0, 2, 1, 1] = 5.0, 10.0          # ... but these two
    sel = heads.transfusion_select_proposals(logits, torch.zeros(1, 4, 9), torch.zeros(1, 9, 2), 8, 3, "other")
    flat = (sel.top_proposals_class * 9 + sel.top_proposals_index)[0].tolist()
    assert flat == [22, 4, 0, 1, 2, 3, 5, 6] and sel.top_proposals_score[0, 2:].eq(0).all()
    assert sel.query_heatmap_score[0, :, 0].tolist() == [float(torch.tensor(5.0).sigmoid()), 0.0, float(torch.tensor(10.0).sigmoid())]


@pytest.mark.parametrize("case", list(gen.DECODE_CASES))
def test_host_get_bboxes_matches_the_reference(case, gold):
    preds, labels = decode_case(case, gold)
    before = {k: v.clone() for k, v in preds.items()}
    res = get_bboxes(case, preds, labels)
    assert all(torch.equal(preds[k], before[k]) for k in preds), "the inputs were modified"
    padded = get_bboxes(case, preds, labels, sync=False)
    for i, rows in enumerate(kept_rows(case, gold)):
        assert same_bits(res[i]["bboxes"].numpy(), gold[case + ".boxes"][i][rows]), "boxes differ from the reference's bits"
        assert same_bits(res[i]["scores"].numpy(), gold[case + ".scores"][i][rows])
        assert np.array_equal(res[i]["labels"].numpy(), gold[case + ".labels"][i][rows]) and res[i]["labels"].dtype == torch.int64
        assert np.array_equal(np.nonzero(padded["keep"][i].numpy())[0], rows) and int(padded["counts"][i]) == len(rows)
    assert same_bits(padded["bboxes"].numpy(), gold[case + ".boxes"]) and same_bits(padded["scores"].numpy(), gold[case + ".scores"])
    assert padded["bboxes"].shape[-1] == (9 if gen.DECODE_CASES[case]["vel"] else 7)


def test_host_coder_decode_matches_the_reference(gold):
    case = "dec_vel_thr_none"
    preds, labels = decode_case(case, gold)
    score = preds["heatmap"].sigmoid() * preds["query_heatmap_score"] * torch.nn.functional.one_hot(labels, 10).permute(0, 2, 1)
    coder = make_coder(0.1)
    res = coder.decode(score, preds["rot"], preds["dim"], preds["center"], preds["height"], preds["vel"])
    assert same_bits(torch.stack([r["bboxes"] for r in res]).numpy(), gold[case + ".boxes"])
    assert np.array_equal(torch.stack([r["labels"] for r in res]).numpy(), gold[case + ".labels"])
    res = coder.decode(score, preds["rot"], preds["dim"], preds["center"], preds["height"], preds["vel"], filter=True)
    for i, rows in enumerate(kept_rows(case, gold)):
        assert same_bits(res[i]["bboxes"].numpy(), gold[case + ".boxes"][i][rows])
    assert coder.post_center_range == gen.CODER["post_center_range"]          # not turned into a tensor
    with pytest.raises(NotImplementedError):
        heads.TransFusionBBoxCoder([-54, -54], 8, [0.075, 0.075]).decode(score, preds["rot"], preds["dim"], preds["center"],
                                                                          preds["height"], None, filter=True)


@pytest.mark.parametrize("case", list(gen.NMS_CASES))
def test_host_circle_nms_matches_the_reference(case, gold):
    dets, pms = nms_case(case, gold), gen.NMS_CASES[case]["pms"]
    keep = heads.circle_nms(dets, gen.RADIUS, pms)
    assert isinstance(keep, list) and keep == gold[case + ".keep"].tolist()
    t = heads.circle_nms(torch.from_numpy(dets), gen.RADIUS, post_max_size=pms)
    assert t.dtype == torch.int64 and t.tolist() == keep
    if pms == 83 and len(dets) > 1:
        assert heads.circle_nms(dets, gen.RADIUS) == keep                     # the reference's default
        assert sorted(heads.circle_nms(dets, -1.0, 10 ** 6)) == list(range(len(dets)))


def test_equal_scores_keep_the_lower_row():
    dets = np.array([[0, 0, 0.5], [0.1, 0, 0.5], [5, 5, 0.5], [0.1, 0.1, 0.9]], np.float32)
    assert heads.circle_nms(dets, 0.175) == [3, 2]
    assert heads.circle_nms(dets[:3], 0.175) == [0, 2]


# ---- registry, coder ---------------------------------------------------------------------------------------------------------
def test_coder_builds_from_the_flagship_config():
    cfg = dict(type="TransFusionBBoxCoder", pc_range=[-54.0, -54.0], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
               score_threshold=0.0, out_size_factor=8, voxel_size=[0.075, 0.075], code_size=10)
    coder = BBOX_CODERS.build(cfg)
    assert isinstance(coder, heads.TransFusionBBoxCoder) and coder.code_size == 10 and coder.out_size_factor == 8
    assert "TransFusionBBoxCoder" in BBOX_CODERS and heads.BBOX_CODERS is BBOX_CODERS


def test_encode_decode_round_trip():
    rng = np.random.default_rng(5)
    n = 40
    boxes = np.concatenate([rng.uniform(-50, 50, (n, 2)), rng.uniform(-3, 1, (n, 1)), rng.uniform(0.3, 6, (n, 3)),
                            rng.uniform(-3.1, 3.1, (n, 1)), rng.uniform(-4, 4, (n, 2))], 1).astype(np.float32)
    coder = make_coder()
    t = coder.encode(torch.from_numpy(boxes))
    assert t.shape == (n, 10)
    col = lambda a, b: t[:, a:b].t()[None].contiguous()   # noqa: E731
    res = coder.decode(torch.rand(1, 10, n), col(6, 8), col(3, 6), col(0, 2), col(2, 3), col(8, 10))
    assert np.allclose(res[0]["bboxes"].numpy(), boxes, rtol=1e-5, atol=1e-4)
    assert heads.TransFusionBBoxCoder([-54, -54], 8, [0.075, 0.075]).encode(torch.from_numpy(boxes)).shape == (n, 8)


# ---- C ABI: arguments are checked before any GPU work ----------------------------------------------------------------------
def test_argument_errors_of_the_entry_points():
    lib = _capi.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.bevamd_head_proposals_workspace_bytes(8, 10, 180, 180) >= 8 * 324000 * 8
    assert lib.bevamd_head_proposals_workspace_bytes(0, 10, 180, 180) == 0 and lib.bevamd_head_proposals_workspace_bytes(1, 70000, 180, 180) == 0
    for args, msg in (((2, 10, 24, 24, 3, 0, 0), "num_proposals"), ((2, 10, 24, 24, 3, 0, 1025), "num_proposals"),
                      ((2, 10, 24, 24, 2, 0, 8), "kernel size"), ((2, 10, 2, 24, 3, 0, 8), "kernel size"),
                      ((0, 10, 24, 24, 3, 0, 8), "bad sizes"), ((1, 1, 2, 2, 1, 0, 5), "num_proposals")):
        assert lib.bevamd_head_proposals(p, *args, p, p, p, p, 1 << 30, None) == 1 and msg in _capi.last_error(), args
    assert lib.bevamd_head_proposals(None, 2, 10, 24, 24, 3, 0, 8, p, p, p, p, 1 << 30, None) == 1 and "null" in _capi.last_error()
    assert lib.bevamd_head_proposals(p, 2, 10, 24, 24, 3, 0, 8, p, p, p, p, 16, None) == 2 and "workspace" in _capi.last_error()

    assert lib.bevamd_head_gather_queries(p, 2, 10, 24, 24, 3, 0, p, 8, p, 3, 16, p, 1, p, p, p, None) == 1 and "feat_dtype" in _capi.last_error()
    assert lib.bevamd_head_gather_queries(p, 2, 10, 24, 24, 3, 0, p, 8, p, 0, 16, p, 3, p, p, p, None) == 1 and "bev_pos" in _capi.last_error()
    assert lib.bevamd_head_gather_queries(p, 2, 10, 24, 24, 3, 0, p, 8, None, 0, 16, p, 1, p, p, p, None) == 1 and "null" in _capi.last_error()

    dec = lambda *a: lib.bevamd_transfusion_decode(*a)   # noqa: E731
    assert dec(p, p, p, p, p, None, p, p, 2, 10, 32, 16, p, p, 0.0, 0, p, p, p, p, None) == 1 and "bad sizes" in _capi.last_error()
    assert dec(p, p, p, p, p, None, p, p, 2, 10, 32, 32, None, p, 0.0, 0, p, p, p, p, None) == 1 and "coder" in _capi.last_error()
    assert dec(p, p, p, p, p, None, p, None, 2, 10, 32, 32, p, p, 0.0, 0, p, p, p, p, None) == 1 and "together" in _capi.last_error()
    assert dec(p, p, None, p, p, None, p, p, 2, 10, 32, 32, p, p, 0.0, 0, p, p, p, p, None) == 1 and "null" in _capi.last_error()

    assert lib.bevamd_circle_nms(p, p, -1, p, 1, p, 10, 83, None, p, None, p, None) == 1 and "bad sizes" in _capi.last_error()
    assert lib.bevamd_circle_nms(p, p, 2000, p, 1, p, 2000, 83, None, p, None, p, None) == 4 and "not supported" in _capi.last_error()
    assert lib.bevamd_circle_nms(p, p, 10, None, 1, p, 10, 83, None, p, None, p, None) == 1 and "segment table" in _capi.last_error()
    assert lib.bevamd_circle_nms(p, p, 10, p, 0, p, 10, 83, None, p, None, p, None) == 0      # no segments: nothing to do


def test_wrapper_argument_errors():
    z = torch.zeros
    with pytest.raises(RuntimeError, match="num_proposals"):
        heads.transfusion_select_proposals(z(1, 10, 8, 8), z(1, 4, 64), z(1, 64, 2), 2000)
    with pytest.raises(RuntimeError, match="nms_kernel_size"):
        heads.transfusion_select_proposals(z(1, 10, 8, 8), z(1, 4, 64), z(1, 64, 2), 8, 2)
    with pytest.raises(ValueError, match="exempts"):
        heads.transfusion_select_proposals(z(1, 3, 8, 8), z(1, 4, 64), z(1, 64, 2), 8, 3, "nuScenes")
    with pytest.raises(RuntimeError, match="needs GPU tensors"):
        heads.circle_nms_segments(z(4, 2), z(4), z(2, dtype=torch.int32), z(1), 4)
    preds, labels = {k: torch.from_numpy(v) for k, v in gen.decode_inputs("dec_novel_nothr_none")[0].items()}, None
    with pytest.raises(ValueError, match="nms_type"):
        heads.transfusion_get_bboxes(preds, labels, make_coder(), dict(dataset="nuScenes", nms_type="soft"), 32, 10)
