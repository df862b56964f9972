"""GPU: the category-encoding kernel, the fused prediction heads and TransFusionHead as a module, against
tests/golden/transfusion_head_ref.npz (the REFERENCE's FFN and forward_single, fp32 and float64, recorded on CPU torch by
tests/golden/make_transfusion_head_golden.py).

Bars.  An output is held to max |got - float64| / max |float64| <= 4 x e_ref, e_ref being the reference's own fp32 deviation from
its float64 recomputation of that output, normalised the same way: per head for the FFN, per entry of the output dict for the
module.  The factor covers another order of the 128-term sums and the BatchNorm folded into a scale and a shift.  Shapes the golden
does not hold are compared with a float64 recomputation of the same formula in numpy, normalised by that output's own largest
magnitude.  The golden's own weights at another P (1, 16, 33) are held, head by head, to that head's golden bar.  Other weights (a
single head, Cin = 4) are held to the SMALLEST of the golden's six bars: their sums are no longer than the golden's, so their
rounding error is no larger.  The one
case at the kernel's limits (Cin = 256, head_conv = 128: both sums twice as long as the golden's) is held to twice that bar, the
worst-case error bound of an fp32 sum being linear in its length.  The
category encoding is one fp32 addition of a rounded fp32 sum: it is held to bit equality with the host formula.  Every observed
figure is recorded next to its bar through conftest.record_parity."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from bevfusion_amd import heads, transfusion_head as th
from conftest import record_parity
from guarded import Arena

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_transfusion_head_golden", os.path.join(HERE, "golden", "make_transfusion_head_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
GOLD = np.load(os.path.join(HERE, "golden", "transfusion_head_ref.npz"))
BAR_FACTOR = 4.0
FILL = 0xA5
BBOX_CODER = dict(type="TransFusionBBoxCoder", pc_range=[-54.0, -54.0], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                  score_threshold=0.0, out_size_factor=8, voxel_size=[0.075, 0.075], code_size=10)


def deviation(got, ref64):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref64).max() / np.abs(ref64).max())


def ffn_bars():
    return {name: BAR_FACTOR * deviation(GOLD[f"ffn.out32.{name}"], GOLD[f"ffn.out64.{name}"]) for name in gen.FFN_HEADS}


def make_ffn(in_channels, ffn_heads, head_conv, seed, dev):
    ffn = th.FFN(in_channels, dict(ffn_heads), head_conv=head_conv)
    shapes = [(k, tuple(v.shape)) for k, v in ffn.state_dict().items()]
    w = gen.weights(shapes, seed)
    ffn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    return ffn.eval().to(dev), w


def ffn_float64(w, ffn_heads, x, query_pos=None, eps=1e-5):
    """The reference's formula in numpy float64 from the unfolded parameters: conv -> BatchNorm (running statistics) -> ReLU -> conv."""
    x = np.asarray(x, np.float64)
    out = {}
    for name in ffn_heads:
        g = lambda key: np.asarray(w[f"{name}.{key}"], np.float64)   # noqa: E731
        hid = np.einsum("jk,bkp->bjp", g("0.conv.weight")[:, :, 0], x)
        hid = (hid - g("0.bn.running_mean")[None, :, None]) / np.sqrt(g("0.bn.running_var") + eps)[None, :, None]
        hid = np.maximum(hid * g("0.bn.weight")[None, :, None] + g("0.bn.bias")[None, :, None], 0.0)
        out[name] = np.einsum("cj,bjp->bcp", g("1.weight")[:, :, 0], hid) + g("1.bias")[None, :, None]
        if name == "center" and query_pos is not None:
            out[name] = out[name] + np.asarray(query_pos, np.float64).transpose(0, 2, 1)
    return out


@pytest.fixture(scope="module")
def golden_ffn(dev):
    ffn, w = make_ffn(gen.FFN_IN, gen.FFN_HEADS, gen.FFN_HEAD_CONV, gen.FFN_SEED, dev)
    assert gen.digest(gen.ffn_inputs(), w) == str(GOLD["ffn.inputs_sha256"]), "inputs and weights do not rebuild the fixture's bytes"
    return ffn, w


def build_head(tag, dev, **extra):
    head = th.TransFusionHead(**gen.head_kwargs(tag), **extra)
    shapes = [(k, tuple(v.shape)) for k, v in head.state_dict().items()]
    w = gen.weights(shapes, int(GOLD[tag + ".seed"]))
    assert gen.digest(gen.head_inputs(tag), w) == str(GOLD[tag + ".inputs_sha256"]), "inputs and weights do not rebuild the fixture's bytes"
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    return head.eval().to(dev)


# ---- category encoding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, C, K, classes, bad", [(2, 128, 17, 10, None), (2, 128, 1, 10, None), (3, 4, 17, 10, None), (2, 128, 17, 10, 10),
                                                   (2, 128, 17, 10, -1)])
def test_class_encoding_is_bit_equal_to_the_host_formula(dev, B, C, K, classes, bad):
    rng = np.random.default_rng(B * 1000 + C * 10 + K)
    q = torch.from_numpy(rng.standard_normal((B, C, K)).astype(np.float32))
    labels = torch.from_numpy(rng.integers(0, classes, (B, K)).astype(np.int64))
    weight = torch.from_numpy(rng.standard_normal((C, classes, 1)).astype(np.float32))
    bias = torch.from_numpy(rng.standard_normal(C).astype(np.float32))
    safe = labels.clone()
    if bad is not None:
        labels[B - 1, K // 2] = bad                      # F.one_hot raises there: the kernel adds nothing to that query
    enc = weight[:, :, 0].t()[safe].permute(0, 2, 1) + bias[None, :, None]       # fp32: weight[c, label] + bias[c], rounded once
    want = q + enc
    if bad is not None:
        want[B - 1, :, K // 2] = q[B - 1, :, K // 2]
    arena = Arena(dev, FILL, capacity=4 << 20)
    gq, gl, gw, gb = arena.put(q, "query_feat"), arena.put(labels, "labels"), arena.put(weight, "weight"), arena.put(bias, "bias")
    got = th.head_class_encoding(gq, gl, gw, gb)
    arena.check()                                        # nothing outside [B, C, K]
    assert got.data_ptr() == gq.data_ptr() and torch.equal(got.cpu(), want)
    assert torch.equal(gl.cpu(), labels) and torch.equal(gw.cpu(), weight) and torch.equal(gb.cpu(), bias)


# ---- the fused prediction heads ----------------------------------------------------------------------------------------------------
def test_ffn_kernel_against_the_float64_golden(dev, golden_ffn):
    ffn, _ = golden_ffn
    x = torch.from_numpy(gen.ffn_inputs()).to(dev)
    with torch.no_grad():
        assert ffn.fusable(x)
        got = ffn(x)
        again = ffn(x)
    assert list(got) == list(gen.FFN_HEADS)
    failures = []
    for name, bar in ffn_bars().items():
        assert tuple(got[name].shape) == GOLD[f"ffn.out64.{name}"].shape
        err = deviation(got[name], GOLD[f"ffn.out64.{name}"])
        record_parity(f"transfusion_head/ffn_kernel/{name}", err, bar)
        print(f"ffn kernel {name}: observed {err:.3e}, bar {bar:.3e}")
        if err > bar:
            failures.append((name, err, bar))
        assert torch.equal(got[name], again[name]), "two equal calls differ"
    assert not failures, failures


CUSTOM = {
    "one_head_one_channel": dict(cin=128, hc=64, heads=dict(height=(1, 2)), P=17),
    "cin4_hc16": dict(cin=4, hc=16, heads=dict(center=(2, 2), dim=(3, 2)), P=17),
    "cin256_hc128_c32": dict(cin=256, hc=128, heads=dict(center=(2, 2), heatmap=(32, 2)), P=19, bar_scale=2.0),
}


@pytest.mark.parametrize("case", ["P1", "P16", "P33", "one_head_one_channel", "cin4_hc16", "cin256_hc128_c32"])
@pytest.mark.parametrize("with_pos", [False, True])
def test_ffn_kernel_shapes_against_float64(dev, golden_ffn, case, with_pos):
    if case in CUSTOM:
        c = CUSTOM[case]
        ffn_heads, P = c["heads"], c["P"]
        ffn, w = make_ffn(c["cin"], ffn_heads, c["hc"], 77, dev)
    else:
        (ffn, w), ffn_heads, P = golden_ffn, gen.FFN_HEADS, int(case[1:])
    with_pos = with_pos and "center" in ffn_heads
    rng = np.random.default_rng(P * 7 + len(ffn_heads))
    x = rng.standard_normal((2, ffn.in_channels, P)).astype(np.float32)
    qpos = rng.uniform(0, 180, (2, P, 2)).astype(np.float32) if with_pos else None
    want = ffn_float64(w, ffn_heads, x, qpos)
    with torch.no_grad():
        xd = torch.from_numpy(x).to(dev)
        assert ffn.fusable(xd)
        got = ffn(xd, None if qpos is None else torch.from_numpy(qpos).to(dev))
    own = ffn_bars()
    failures = []
    for name in ffn_heads:
        assert tuple(got[name].shape) == want[name].shape
        err = deviation(got[name], want[name])
        bar = min(own.values()) * CUSTOM[case].get("bar_scale", 1.0) if case in CUSTOM else own[name]
        record_parity(f"transfusion_head/ffn_kernel_{case}{'_pos' if with_pos else ''}/{name}", err, bar)
        if err > bar:
            failures.append((name, err, bar))
    assert not failures, failures


@pytest.mark.parametrize("P, stride, offset", [(17, 17, 0), (17, 34, 17), (17, 34, 0), (16, 49, 33), (1, 3, 1)])
def test_ffn_kernel_writes_its_columns_and_nothing_else(dev, golden_ffn, P, stride, offset):
    """Guarded buffers: every input and output has the exact size the header promises; the columns outside
    [offset, offset + P) keep the sentinel, the guards around every buffer stay whole, and the written columns equal an unguarded
    call's bit for bit."""
    ffn, w = golden_ffn
    rng = np.random.default_rng(P)
    x = torch.from_numpy(rng.standard_normal((2, gen.FFN_IN, P)).astype(np.float32))
    qpos = torch.from_numpy(rng.uniform(0, 180, (2, P, 2)).astype(np.float32))
    names = list(gen.FFN_HEADS)
    with torch.no_grad():
        plain = ffn(x.to(dev), qpos.to(dev))
    arena = Arena(dev, FILL, capacity=8 << 20)
    params = [tuple(arena.put(t, f"{name}.{i}") for i, t in enumerate(p)) for name, p in zip(names, ffn.folded())]
    gx, gpos = arena.put(x, "x"), arena.put(qpos, "query_pos")
    outs = [arena.out((2, gen.FFN_HEADS[name][0], stride), torch.float32, name) for name in names]
    res = th.head_ffn_forward(gx, params, gpos, names.index("center"), outs, offset)
    assert res is not None
    arena.check()
    for name, o in zip(names, outs):
        assert torch.equal(o[..., offset:offset + P], plain[name]), name
        arena.untouched(o[..., :offset])
        arena.untouched(o[..., offset + P:])
    assert torch.equal(gx.cpu(), x) and torch.equal(gpos.cpu(), qpos)


def test_ffn_module_falls_back_to_its_torch_layers_only_where_documented(dev, golden_ffn):
    ffn, _ = golden_ffn
    x = torch.from_numpy(gen.ffn_inputs()).to(dev)
    with torch.no_grad():
        fused = ffn(x)
        ffn.use_fused = False
        try:
            assert not ffn.fusable(x)
            torch_path = ffn(x)
        finally:
            ffn.use_fused = True
    assert not ffn.fusable(x)                            # gradients enabled and the parameters require them
    for name, bar in ffn_bars().items():
        assert deviation(torch_path[name], GOLD[f"ffn.out64.{name}"]) <= bar
        assert deviation(fused[name], GOLD[f"ffn.out64.{name}"]) <= bar


# ---- the module --------------------------------------------------------------------------------------------------------------------
def entry_bars(tag):
    return {str(k): BAR_FACTOR * deviation(GOLD[f"{tag}.out32.{k}"], GOLD[f"{tag}.out64.{k}"]) for k in GOLD[tag + ".keys"]}


@pytest.fixture(scope="module", params=["single", "aux"])
def head_case(request, dev):
    tag = request.param
    head = build_head(tag, dev, bbox_coder=dict(BBOX_CODER))
    x = torch.from_numpy(gen.head_inputs(tag)).to(dev)
    return tag, head, x


def check_outputs(tag, out, label):
    failures = []
    assert list(out) == [str(k) for k in GOLD[tag + ".keys"]]
    for key, bar in entry_bars(tag).items():
        ref = GOLD[f"{tag}.out64.{key}"]
        assert tuple(out[key].shape) == ref.shape, key
        err = deviation(out[key], ref)
        record_parity(f"transfusion_head/{tag}/{label}/{key}", err, bar)
        print(f"{tag} {label} {key}: observed {err:.3e}, bar {bar:.3e}")
        if err > bar:
            failures.append((key, err, bar))
    assert not failures, failures


def test_head_forward_selects_the_golden_proposals_and_meets_its_bars(head_case):
    tag, head, x = head_case
    with torch.no_grad():
        res = head(x)
    assert isinstance(res, list) and len(res) == 1 and isinstance(res[0], list) and len(res[0]) == 1
    out = res[0][0]
    assert torch.equal(head.query_labels.cpu(), torch.from_numpy(GOLD[tag + ".proposal_class"]))
    # the selection is a function of dense_heatmap alone: run on the forward's own map, it names the forward's proposals
    sel = heads.transfusion_select_proposals(out["dense_heatmap"], torch.zeros((gen.B, 1, gen.BEV * gen.BEV), device=x.device), head.bev_pos,
                                             gen.PROPOSALS, 3, "nuScenes")
    assert torch.equal(sel.top_proposals_class, head.query_labels)
    assert torch.equal(sel.top_proposals_index.cpu(), torch.from_numpy(GOLD[tag + ".proposal_index"]))
    assert torch.equal(sel.query_heatmap_score, out["query_heatmap_score"])
    check_outputs(tag, out, "fused")


def test_head_forward_without_the_fused_kernels_meets_the_same_bars(head_case):
    tag, head, x = head_case
    head.use_fused = False
    try:
        with torch.no_grad():
            out = head(x)[0][0]
    finally:
        head.use_fused = True
    assert torch.equal(head.query_labels.cpu(), torch.from_numpy(GOLD[tag + ".proposal_class"]))
    check_outputs(tag, out, "torch")


def test_head_auxiliary_false_returns_the_last_layer(dev):
    head = build_head("aux", dev)
    x = torch.from_numpy(gen.head_inputs("aux")).to(dev)
    with torch.no_grad():
        head.auxiliary = False
        last = head(x)[0][0]
    P = gen.PROPOSALS
    assert sorted(last) == sorted(["center", "height", "dim", "rot", "vel", "heatmap"])  # the reference attaches the rest to layer 0
    bars = entry_bars("aux")
    for key in last:
        ref = GOLD[f"aux.out64.{key}"]
        assert tuple(last[key].shape) == ref[..., P:].shape
        # the bar of the whole entry, normalised by the whole entry's largest magnitude as the bar is
        err = float(np.abs(last[key].cpu().double().numpy() - ref[..., P:]).max() / np.abs(ref).max())
        record_parity(f"transfusion_head/aux/last_layer_only/{key}", err, bars[key])
        assert err <= bars[key], (key, err, bars[key])


def test_head_train_mode_backpropagates(dev):
    head = build_head("single", dev).train()
    x = torch.from_numpy(gen.head_inputs("single")).to(dev)
    torch.manual_seed(3)
    out = head(x)[0][0]
    loss = sum(out[k].float().square().mean() for k in ("center", "height", "dim", "rot", "vel", "heatmap", "dense_heatmap"))
    loss.backward()
    for p in (head.shared_conv.weight, head.prediction_heads[0].center[0].conv.weight, head.prediction_heads[0].heatmap[1].bias,
              head.class_encoding.weight, head.decoder[0].linear1.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
    assert int(head.prediction_heads[0].center[0].bn.num_batches_tracked) == 8         # the torch layers ran on batch statistics


def test_head_forward_replays_under_a_graph(head_case):
    tag, head, x = head_case
    rng = np.random.default_rng(11)
    fresh = lambda: x + torch.from_numpy(rng.standard_normal(tuple(x.shape)).astype(np.float32) * 1e-3).to(x.device)   # noqa: E731
    static = x.clone()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            head(static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                     # a capture admits no sync and no read-back
            out = head(static)[0][0]
            labels = head.query_labels
        for _ in range(2):
            contents = fresh()
            static.copy_(contents)
            graph.replay()
            torch.cuda.synchronize()
            eager = head(contents)[0][0]
            assert torch.equal(labels, head.query_labels)
            for key in eager:
                assert torch.equal(out[key], eager[key]), key


def test_head_get_bboxes_equals_the_function(head_case):
    tag, head, x = head_case
    saved = head.test_cfg
    try:
        with torch.no_grad():
            res = head(x)
            for nms_type in (None, "circle"):
                cfg = dict(saved, nms_type=nms_type)
                head.test_cfg = cfg
                got = head.get_bboxes(res)
                want = heads.transfusion_get_bboxes(res[0][0], head.query_labels, head.bbox_coder, cfg, gen.PROPOSALS, gen.CLASSES)
                assert len(got) == len(want) == gen.B
                for g, w in zip(got, want):
                    assert sorted(g) == ["bboxes", "labels", "scores"] and g["bboxes"].shape[0] > 0
                    for key in g:
                        assert torch.equal(g[key], w[key])
            # metas with a box type: every sample's boxes are wrapped with the width of the code, labels become int32
            wrapped = head.get_bboxes(res, [dict(box_type_3d=lambda t, box_dim: ("boxes", t, box_dim)) for _ in range(gen.B)])
            assert len(wrapped) == gen.B
            for (boxes, scores, labels), w in zip(wrapped, want):
                assert boxes[0] == "boxes" and boxes[2] == 9 and torch.equal(boxes[1], w["bboxes"])
                assert torch.equal(scores, w["scores"]) and labels.dtype == torch.int32 and torch.equal(labels.long(), w["labels"])
            plain = head.get_bboxes(res, [dict() for _ in range(gen.B)])          # metas without a box type: bare tensors
            assert all(torch.equal(p[0], w["bboxes"]) for p, w in zip(plain, want))
    finally:
        head.test_cfg = saved


TRAIN_CFG = dict(dataset="nuScenes", point_cloud_range=[-54.0, -54.0, -5.0, -46.8, -46.8, 3.0], grid_size=[gen.BEV * 8, gen.BEV * 8, 1],
                 voxel_size=[0.075, 0.075, 8.0], out_size_factor=8, gaussian_overlap=0.1, min_radius=2, pos_weight=-1,
                 code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2],
                 assigner=dict(type="HungarianAssigner3D", iou_calculator=dict(type="BboxOverlaps3D", coordinate="lidar"),
                               cls_cost=dict(type="FocalLossCost", gamma=2.0, alpha=0.25, weight=0.15),
                               reg_cost=dict(type="BBoxBEVL1Cost", weight=0.25), iou_cost=dict(type="IoU3DCost", weight=0.25)))


def test_head_get_targets_and_loss_are_the_functions_on_the_heads_own_settings(dev):
    """`head.get_targets` / `head.loss` against `transfusion_get_targets` / `transfusion_loss` called here with every argument by
    name from the config: the methods pass the right thing in the right place.  Two decoder layers, auxiliary."""
    head = build_head("aux", dev, bbox_coder=dict(BBOX_CODER), train_cfg=dict(TRAIN_CFG))
    assert isinstance(head.bbox_assigner, heads.HungarianAssigner3D)
    x = torch.from_numpy(gen.head_inputs("aux")).to(dev)
    rng = np.random.default_rng(21)
    gt_boxes, gt_labels = [], []
    for n in (3, 5):
        xy = rng.uniform(-53.0, -47.8, (n, 2))
        rest = np.concatenate([rng.uniform(-1.0, 1.0, (n, 1)), rng.uniform(0.6, 2.5, (n, 3)), rng.uniform(-3.0, 3.0, (n, 1)),
                               rng.uniform(-1.0, 1.0, (n, 2))], axis=1)
        gt_boxes.append(torch.from_numpy(np.concatenate([xy, rest], axis=1).astype(np.float32)).to(dev))
        gt_labels.append(torch.from_numpy(rng.integers(0, gen.CLASSES, n).astype(np.int64)).to(dev))
    preds = head(x)                                          # eval mode, gradients on: the torch layers, a graph to the parameters
    targets = head.get_targets(gt_boxes, gt_labels, preds[0])
    want_targets = heads.transfusion_get_targets(gt_boxes, gt_labels, preds[0][0], bbox_coder=head.bbox_coder, assigner=head.bbox_assigner,
                                                 train_cfg=TRAIN_CFG, num_proposals=gen.PROPOSALS, num_classes=gen.CLASSES,
                                                 num_decoder_layers=2, auxiliary=True)
    assert len(targets) == len(want_targets) == 8 and targets[5] == want_targets[5] > 0      # num_pos: something was matched
    for got, want in zip(targets, want_targets):
        assert torch.equal(got, want) if torch.is_tensor(got) else got == want
    assert tuple(targets[0].shape) == (gen.B, 2 * gen.PROPOSALS) and tuple(targets[7].shape) == (gen.B, gen.CLASSES, gen.BEV, gen.BEV)
    losses = head.loss(gt_boxes, gt_labels, preds)
    kw = gen.head_kwargs("aux")
    want = heads.transfusion_loss(preds[0][0], want_targets, num_proposals=gen.PROPOSALS, num_classes=gen.CLASSES, num_decoder_layers=2,
                                  auxiliary=True, code_weights=TRAIN_CFG["code_weights"], loss_cls=kw["loss_cls"],
                                  loss_bbox=kw["loss_bbox"], loss_heatmap=kw["loss_heatmap"])
    assert sorted(losses) == sorted(want) == sorted(["loss_heatmap", "layer_0_loss_cls", "layer_0_loss_bbox", "layer_-1_loss_cls",
                                                      "layer_-1_loss_bbox", "matched_ious"])
    for key in want:
        assert torch.equal(losses[key], want[key]) and bool(torch.isfinite(losses[key]).all()), key
    sum(v for k, v in losses.items() if k != "matched_ious").backward()
    for p in (head.shared_conv.weight, head.prediction_heads[1].center[0].conv.weight, head.prediction_heads[0].heatmap[1].bias):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
