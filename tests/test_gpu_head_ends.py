"""GPU: the TransFusion head-end kernels (csrc/ext/head_ends.hip) against tests/golden/head_ends_ref.npz (the REFERENCE on CPU
torch, see tests/golden/make_head_ends_golden.py) and, where the reference leaves the order open, against the host formulation
with a stable argsort.

Bars: classes, indices, labels, valid and keep sets exactly equal; top_score and query_heatmap_score within 2 ulp (two
evaluations of the sigmoid); query_feat / query_pos bit-equal (copies); the centre and velocity columns of the boxes bit-equal
(same fp32 operations, no FMA contraction); dim, yaw, height and score columns within 4 x the reference CPU result's own maximum
error against the fixture's float64 values, per column, with a floor of 2 ulp of the column's largest magnitude."""
import numpy as np
import pytest
import torch

from bevfusion_amd import heads
from conftest import record_parity
from test_head_ends import decode_case, gen, get_bboxes, gold, kept_rows, make_coder, nms_case, same_bits, select, selection_case  # noqa: F401

pytestmark = pytest.mark.gpu


def check_against_host(logits, K, k=3, dataset="nuScenes", Cf=4):
    """Every output of the device selection equals the host formulation (stable argsort) exactly; scores within 2 ulp."""
    B, C, H, W = logits.shape
    rng = np.random.default_rng(9)
    feat = torch.from_numpy(rng.standard_normal((B, Cf, H * W)).astype(np.float32))
    pos = torch.from_numpy(rng.standard_normal((B, H * W, 2)).astype(np.float32))
    want = heads.transfusion_select_proposals(logits, feat, pos, K, k, dataset)
    got = heads.transfusion_select_proposals(logits.cuda(), feat.cuda(), pos.cuda(), K, k, dataset)
    assert torch.equal(got.top_proposals_class.cpu(), want.top_proposals_class)
    assert torch.equal(got.top_proposals_index.cpu(), want.top_proposals_index)
    assert gen.ulps(got.top_proposals_score.cpu().numpy(), want.top_proposals_score.numpy()).max() <= 2
    assert gen.ulps(got.query_heatmap_score.cpu().numpy(), want.query_heatmap_score.numpy()).max() <= 2
    assert torch.equal(got.query_feat.cpu(), want.query_feat) and torch.equal(got.query_pos.cpu(), want.query_pos)
    return got


@pytest.mark.parametrize("case", list(gen.SELECTION_CASES))
def test_selection_matches_the_reference(case, gold, dev):
    sel = select(case, selection_case(case, gold, dev))
    assert np.array_equal(sel.top_proposals_class.cpu().numpy(), gold[case + ".top_class"])
    assert np.array_equal(sel.top_proposals_index.cpu().numpy(), gold[case + ".top_index"])
    u_top = int(gen.ulps(sel.top_proposals_score.cpu().numpy(), gold[case + ".top_score"]).max())
    u_q = int(gen.ulps(sel.query_heatmap_score.cpu().numpy(), gold[case + ".query_heatmap_score"]).max())
    print(f"{case}: top_score {u_top} ulp, query_heatmap_score {u_q} ulp (bar 2)")
    record_parity(f"head_ends/{case}/top_score_ulp", u_top, 2)
    record_parity(f"head_ends/{case}/query_heatmap_score_ulp", u_q, 2)
    assert u_top <= 2 and u_q <= 2
    assert gen.sha(sel.query_feat.cpu().numpy()) == str(gold[case + ".query_feat_sha256"])
    assert gen.sha(sel.query_pos.cpu().numpy()) == str(gold[case + ".query_pos_sha256"])
    half = heads.transfusion_select_proposals(*[t.half() if i == 1 else t for i, t in enumerate(selection_case(case, gold, dev))],
                                              num_proposals=32, dataset=gen.SELECTION_CASES[case]["dataset"])
    assert half.query_feat.dtype == torch.float16 and torch.equal(half.query_feat.float(), sel.query_feat.half().float())


def test_ties_come_in_ascending_flat_index(dev):
    """Logits from an 8-value set: most of the top K tie."""
    rng = np.random.default_rng(21)
    values = np.array([-3, -2, -1, -0.5, 0, 0.5, 1, 2], np.float32)
    logits = torch.from_numpy(values[rng.integers(0, 8, (2, 10, 24, 24))])
    sel = check_against_host(logits, 32)
    assert len(np.unique(sel.top_proposals_score.cpu().numpy())) <= 2
    check_against_host(logits, 1024)


@pytest.mark.parametrize("K", [32, 1024])
def test_fewer_survivors_than_proposals(K, dev):
    """A flat map with 5 peaks on a non-exempt ramp: zeros fill the list in ascending flat index."""
    ramp = -(torch.arange(24.0 * 24).view(24, 24) / 64 + 1)          # strictly decreasing: no interior cell is a window maximum
    logits = ramp.expand(2, 10, 24, 24).clone()
    logits[:, 8:] = -200.0                                         # exempt classes: sigmoid underflows to 0 — zeros as well
    for n, (c, y, x) in enumerate(((0, 3, 3), (2, 10, 12), (5, 20, 5), (7, 1, 22), (7, 22, 1))):
        logits[0, c, y, x] = 1.0 + n
        logits[1, c, 23 - y, x] = 2.0 + n
    sel = check_against_host(logits, K)
    assert sel.top_proposals_score[:, 5:].eq(0).all() and sel.top_proposals_score[:, :5].gt(0.7).all()


@pytest.mark.parametrize("shape,K,k,dataset", [((2, 10, 3, 9), 16, 3, "nuScenes"), ((2, 3, 7, 3), 5, 3, "other"), ((2, 10, 24, 24), 1, 3, "nuScenes"),
                                               ((1, 10, 24, 24), 32, 3, "nuScenes"), ((2, 3, 9, 11), 40, 1, "Waymo"),
                                               ((1, 3, 31, 33), 64, 5, "other")])
def test_selection_edge_shapes(shape, K, k, dataset, dev):
    """H or W equal to k (one interior row / column), K = 1, B = 1, k = 1 (nothing suppressed), k = 5."""
    B, C, H, W = shape
    rng = np.random.default_rng(sum(shape) + K)
    logits = np.stack([(rng.choice(12289, size=C * H * W, replace=False) - 6144) / 1024.0 for _ in range(B)])
    check_against_host(torch.from_numpy(logits.reshape(shape).astype(np.float32)), K, k, dataset)


def column_bars(ref32, ref64):
    """Per column: 4 x the reference's own fp32-vs-float64 error, at least 2 ulp of the column's largest magnitude."""
    e_ref = np.abs(ref32.astype(np.float64) - ref64).reshape(-1, ref32.shape[-1]).max(0)
    floor = 2 * np.spacing(np.abs(ref32).reshape(-1, ref32.shape[-1]).max(0).astype(np.float32)).astype(np.float64)
    return np.maximum(4 * e_ref, floor)


@pytest.mark.parametrize("case", list(gen.DECODE_CASES))
def test_get_bboxes_matches_the_reference(case, gold, dev):
    preds, labels = decode_case(case, gold, dev)
    before = {k: v.clone() for k, v in preds.items()}
    out = get_bboxes(case, preds, labels, sync=False)
    assert all(torch.equal(preds[k], before[k]) for k in preds), "the inputs were modified"
    boxes, scores = out["bboxes"].cpu().numpy(), out["scores"].cpu().numpy()
    ref, ref64 = gold[case + ".boxes"], gold[case + ".boxes64"]
    exact = [0, 1] + ([7, 8] if gen.DECODE_CASES[case]["vel"] else [])
    assert same_bits(boxes[..., exact], ref[..., exact]), "centre / velocity columns differ from the reference's bits"
    bars = column_bars(ref, ref64)
    err = np.abs(boxes.astype(np.float64) - ref64).reshape(-1, ref.shape[-1]).max(0)
    s_bar = column_bars(gold[case + ".scores"][..., None], gold[case + ".scores64"][..., None])[0]
    s_err = float(np.abs(scores.astype(np.float64) - gold[case + ".scores64"]).max())
    names = ["x", "y", "z", "dx", "dy", "dz", "yaw", "vx", "vy"]
    for j in range(ref.shape[-1]):
        print(f"{case} {names[j]}: observed {err[j]:.3e}  bar {bars[j]:.3e}")
        record_parity(f"head_ends/{case}/{names[j]}", err[j], bars[j])
    print(f"{case} score: observed {s_err:.3e}  bar {s_bar:.3e}")
    record_parity(f"head_ends/{case}/score", s_err, s_bar)
    assert np.all(err <= bars) and s_err <= s_bar
    assert np.array_equal(out["labels"].cpu().numpy(), gold[case + ".labels"])
    rows = kept_rows(case, gold)
    for i in range(len(rows)):
        assert np.array_equal(np.nonzero(out["keep"][i].cpu().numpy())[0], rows[i])
    assert out["counts"].tolist() == [len(r) for r in rows]
    res = get_bboxes(case, preds, labels)                                  # sync=True: the reference's list of dicts
    for i in range(len(rows)):
        assert torch.equal(res[i]["bboxes"], out["bboxes"][i][rows[i]]) and torch.equal(res[i]["scores"], out["scores"][i][rows[i]])
        assert torch.equal(res[i]["labels"].cpu(), torch.from_numpy(gold[case + ".labels"][i][rows[i]].astype(np.int64)))


def test_decode_reads_the_last_proposals_and_serves_the_coder(gold, dev):
    case = "dec_vel_thr_none"
    preds, labels = decode_case(case, gold, dev)
    want = get_bboxes(case, preds, labels, sync=False)
    wide = {k: (torch.cat([torch.randn_like(v), v], -1) if k != "query_heatmap_score" else v) for k, v in preds.items()}
    got = get_bboxes(case, wide, labels, sync=False)                       # all decoder layers concatenated: the last K count
    assert all(torch.equal(got[k], want[k]) for k in want)
    coder = make_coder(0.1)
    res = coder.decode(want["scores"][:, None, :].expand(-1, 10, -1).contiguous(), preds["rot"], preds["dim"], preds["center"],
                       preds["height"], preds["vel"], filter=True)
    valid = want["keep"]
    for i in range(2):
        assert torch.equal(res[i]["bboxes"], want["bboxes"][i][valid[i]]) and res[i]["labels"].eq(0).all()


@pytest.mark.parametrize("case", list(gen.NMS_CASES))
def test_circle_nms_matches_the_reference(case, gold, dev):
    dets, pms = torch.from_numpy(nms_case(case, gold)).to(dev), gen.NMS_CASES[case]["pms"]
    keep = heads.circle_nms(dets, gen.RADIUS, pms)
    assert keep.dtype == torch.int64 and keep.is_cuda and keep.tolist() == gold[case + ".keep"].tolist()


def test_segmented_circle_nms_equals_single_calls(gold, dev):
    dets, off, thr = gen.segmented_inputs()
    assert gen.sha(dets, off, thr) == str(gold["segmented.inputs_sha256"])
    d = torch.from_numpy(dets).to(dev)
    pms = 20
    keep, order, counts = heads.circle_nms_segments(d[:, :2], d[:, 2], torch.from_numpy(off).to(dev), torch.from_numpy(thr).to(dev), 300, pms)
    keep, order = keep.cpu().numpy(), order.cpu().numpy()
    for s in range(3):
        rows = np.nonzero(keep[off[s]:off[s + 1]])[0]
        if thr[s] > 0:
            single = heads.circle_nms(d[off[s]:off[s + 1]], float(thr[s]), pms).cpu().numpy()
            assert np.array_equal(order[off[s]:off[s] + len(single)] - off[s], single) and np.array_equal(rows, np.sort(single))
        else:                                                              # every row, no cap
            assert len(rows) == off[s + 1] - off[s] > pms
        assert int(counts[s]) == len(rows)
    # the fixture's recorded sets: segment 0 with the default cap, segment 1 all rows, segment 2
    keep83, _, _ = heads.circle_nms_segments(d[:, :2], d[:, 2], torch.from_numpy(off).to(dev), torch.from_numpy(thr).to(dev), 300)
    rows83 = np.nonzero(keep83.cpu().numpy())[0]
    for s in range(3):
        assert np.array_equal(rows83[(rows83 >= off[s]) & (rows83 < off[s + 1])], gold[f"segmented.keep{s}"])
    live = torch.ones(len(dets), dtype=torch.bool, device=dev)
    best = int(np.argmax(dets[:off[1], 2]))
    live[best] = False                                                     # a dead row takes no part: the runner-up leads
    _, order2, _ = heads.circle_nms_segments(d[:, :2], d[:, 2], torch.from_numpy(off).to(dev), torch.from_numpy(thr).to(dev), 300, pms, live)
    assert int(order2[0]) == int(np.argsort(-dets[:off[1], 2])[1])
    _, _, counts = heads.circle_nms_segments(d[:, :2], d[:, 2], torch.from_numpy(off).to(dev), torch.from_numpy(thr).to(dev), 100, pms)
    assert counts.tolist()[1] == -1 and counts.tolist()[0] > 0              # longer than the caller's bound: reported, nothing kept


def test_selection_and_get_bboxes_replay_in_one_graph(gold, dev):
    case = "dec_vel_nothr_circle"
    c = gen.DECODE_CASES[case]
    static = selection_case("sel_nus", gold, dev)
    preds, _ = decode_case(case, gold, dev)
    coder, cfg = make_coder(c["score_threshold"]), dict(dataset="nuScenes", nms_type="circle")

    def step():
        sel = heads.transfusion_select_proposals(*static, num_proposals=32, nms_kernel_size=3, dataset="nuScenes")
        pd = dict(preds, query_heatmap_score=sel.query_heatmap_score)
        return sel, heads.transfusion_get_bboxes(pd, sel.top_proposals_class, coder, cfg, 32, 10, sync=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                             # warm-up: builds the cached task tables
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sel, out = step()
    rng = np.random.default_rng(77)
    for _ in range(2):
        fresh = np.stack([(rng.choice(12289, size=5760, replace=False) - 6144) / 1024.0 for _ in range(2)]).reshape(2, 10, 24, 24)
        static[0].copy_(torch.from_numpy(fresh.astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (sel.top_proposals_class, sel.top_proposals_index, sel.top_proposals_score, sel.query_feat, sel.query_pos,
                                   sel.query_heatmap_score, out["bboxes"], out["scores"], out["labels"], out["keep"], out["counts"])]
        esel, eout = step()
        want = (esel.top_proposals_class, esel.top_proposals_index, esel.top_proposals_score, esel.query_feat, esel.query_pos,
                esel.query_heatmap_score, eout["bboxes"], eout["scores"], eout["labels"], eout["keep"], eout["counts"])
        assert all(torch.equal(g, w) for g, w in zip(got, want))
