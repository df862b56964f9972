"""GPU: the fused task heads (`bevamd_center_heads_forward`) and CenterHead / SeparateHead as modules, against
tests/golden/centerhead_module_ref.npz (the REFERENCE's SeparateHead and CenterHead.forward_single, fp32 and float64, recorded on
CPU torch by tests/golden/make_centerhead_module_golden.py).

Bars.  An output is held to max |got - float64| / max |float64| <= 4 x e_ref, e_ref being the reference's own fp32 deviation from
its float64 recomputation of that output, normalised the same way, per head.  The factor covers another order of the 576-term sums
and the BatchNorm folded into a scale and a shift.  Maps the golden does not hold are compared with the float64 output of a
`.double()` copy of the same module on the CPU, normalised by that output's own largest magnitude; the golden's weights on another
map are held, head by head, to that head's golden bar.  Other weights (a single head, 16 channels, 8 tasks, 10 classes) are held to
the SMALLEST bar of the golden recording with the same final_kernel: their sums are no longer than the golden's, so their rounding
error is no larger.  A stack of three convolutions (the num_conv = 3 fallback) is held to 1.5 x that bar: three rounded sums in a
row where the golden has two, the error bound of a chain being linear in its depth.  The border rule is checked on small integers,
bit for bit.  Every observed figure is recorded next to its bar through conftest.record_parity."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from bevfusion_amd import centerhead_module as cm, heads
from conftest import record_parity
from guarded import Arena

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_centerhead_module_golden", os.path.join(HERE, "golden", "make_centerhead_module_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
GOLD = np.load(os.path.join(HERE, "golden", "centerhead_module_ref.npz"))
BAR_FACTOR = 4.0
TILE = cm.CH_TILE                 # final_kernel -> output cells (H, W) of one workgroup


def deviation(got, ref64):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref64 = ref64.detach().cpu().double().numpy() if isinstance(ref64, torch.Tensor) else ref64
    assert np.isfinite(got).all()
    return float(np.abs(got - ref64).max() / np.abs(ref64).max())


def bars(tag):
    return {str(k): BAR_FACTOR * deviation(GOLD[f"{tag}.out32.{k}"], GOLD[f"{tag}.out64.{k}"]) for k in GOLD[tag + ".keys"]}


def load_seeded(module, seed):
    shapes = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    w = gen.weights(shapes, seed)
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    return w


def build(tag):
    """(the module on the host in eval mode, loaded with the recording's state)."""
    if tag == "head":
        module = cm.CenterHead(**gen.head_kwargs())
    else:
        module = cm.SeparateHead(64, dict(gen.SEP_HEADS), final_kernel=gen.SEP[tag]["final_kernel"])
    w = load_seeded(module, gen.seed_of(tag))
    assert gen.digest(gen.inputs(tag), w) == str(GOLD[tag + ".inputs_sha256"]), "inputs and weights do not rebuild the fixture's bytes"
    return module.eval()


def flat(module, x):
    if isinstance(module, cm.CenterHead):
        return {f"{t}.{name}": v for t, d in enumerate(module.forward_single(x)) for name, v in d.items()}
    return module(x)


def float64_of(module, x):
    """The float64 output of a .double() copy of a host module on the CPU."""
    with torch.no_grad():
        return flat(copy.deepcopy(module).cpu().double(), x.detach().cpu().double())


def check(label, got, want, bar_of, failures=None):
    own = [] if failures is None else failures
    assert list(got) == list(want)
    for key in want:
        ref = want[key] if isinstance(want[key], np.ndarray) else want[key].numpy()
        assert tuple(got[key].shape) == ref.shape, key
        err, bar = deviation(got[key], ref), bar_of(key)
        record_parity(f"centerhead_module/{label}/{key}", err, bar)
        print(f"{label} {key}: observed {err:.3e}, bar {bar:.3e}")
        if err > bar:
            own.append((label, key, err, bar))
    if failures is None:
        assert not own, own


@pytest.fixture(scope="module", params=["sep3", "sep1"])
def sep(request, dev):
    tag = request.param
    host = build(tag)
    return tag, host, copy.deepcopy(host).to(dev)


# ---- the kernel against the golden -------------------------------------------------------------------------------------------------
def test_kernel_against_the_float64_golden(dev, sep):
    tag, _, head = sep
    x = torch.from_numpy(gen.inputs(tag)).to(dev)
    with torch.no_grad():
        assert head.fusable(x)
        got = head(x)
        again = head(x)
    assert all(v.is_contiguous() for v in got.values())
    check(f"{tag}/kernel", got, {str(k): GOLD[f"{tag}.out64.{k}"] for k in GOLD[tag + ".keys"]}, bars(tag).__getitem__)
    for key in got:
        assert torch.equal(got[key], again[key]), "two equal calls differ"


def map_sizes(k):
    th, tw = TILE[k]
    return [(1, 1), (1, 7), (3, 5), (th, tw), (th + 1, tw), (th, tw + 1), (9, 37)]


@pytest.mark.parametrize("index", range(7))
def test_kernel_on_other_maps_against_float64(dev, sep, index):
    """1 x 1, 1 x 7, 3 x 5, the tile's exact extent, one more than the tile in H and in W, and 9 x 37 (several tiles, not square)."""
    tag, host, head = sep
    H, W = map_sizes(head.final_kernel)[index]
    x = torch.from_numpy(np.random.default_rng(100 * H + W).standard_normal((2, 64, H, W)).astype(np.float32))
    want = float64_of(host, x)
    with torch.no_grad():
        xd = x.to(dev)
        assert head.fusable(xd)
        got = head(xd)
    check(f"{tag}/kernel_{H}x{W}", got, want, bars(tag).__getitem__)


# ---- the border rule, exact --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("H, W", [(9, 17), (1, 1), (2, 3), (7, 15)])
def test_hidden_cells_outside_the_map_are_zero(dev, k, H, W):
    """x = 0, scale 1, a positive integer shift per hidden channel, a final weight of ones and an integer bias: the hidden map is
    `shift` on every cell of the map and ZERO outside it, so an output cell is bias + (taps of its window inside the map) x
    sum(shift): 9 in the interior, 6 on an edge, 4 in a corner of a map at least 2 x 2; 1 everywhere with final_kernel 1.  Small
    integers: compared bit for bit."""
    head = cm.SeparateHead(64, dict(reg=(2, 2), heatmap=(3, 2)), final_kernel=k).eval().to(dev)
    rng = np.random.default_rng(k)
    shifts = [torch.from_numpy(rng.integers(1, 5, 64).astype(np.float32)) for _ in range(2)]
    biases = [torch.tensor([3.0, -2.0]), torch.tensor([0.0, 7.0, -5.0])]
    with torch.no_grad():
        for seq, bias in zip((head.reg, head.heatmap), biases):
            seq[1].weight.fill_(1.0)
            seq[1].bias.copy_(bias)
        folded = head.folded()
        for i in range(2):
            folded.scales[i].fill_(1.0)          # views of the packed buffer
            folded.shifts[i].copy_(shifts[i])
        res = cm.center_heads_forward(torch.zeros(2, 64, H, W, device=dev), folded)[0]
    p = k // 2
    ys, xs = np.arange(H), np.arange(W)
    count = np.outer(np.minimum(ys + p, H - 1) - np.maximum(ys - p, 0) + 1, np.minimum(xs + p, W - 1) - np.maximum(xs - p, 0) + 1)
    if k == 3 and H >= 3 and W >= 3:
        assert count[1, 1] == 9 and count[0, 1] == 6 and count[1, 0] == 6 and count[0, 0] == count[-1, -1] == 4
    for got, shift, bias in zip(res, shifts, biases):
        want = bias.numpy()[None, :, None, None] + float(shift.sum()) * count[None, None].astype(np.float32)
        want = np.broadcast_to(want, got.shape).astype(np.float32)
        assert np.array_equal(got.cpu().numpy(), want), (k, H, W)


# ---- bits --------------------------------------------------------------------------------------------------------------------------
def test_a_sample_does_not_depend_on_its_batch(dev, sep):
    tag, _, head = sep
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((3, 64, 9, 17)).astype(np.float32)).to(dev)
    with torch.no_grad():
        batch = head(x)
        for b in range(3):
            alone = head(x[b:b + 1].contiguous())
            for key in batch:
                assert torch.equal(batch[key][b:b + 1], alone[key]), (key, b)


@pytest.mark.parametrize("fill", [0x00, 0xA5, 0xFF])
@pytest.mark.parametrize("H, W", [(9, 11), (6, 14), (1, 1), (13, 30)])
def test_kernel_writes_its_outputs_and_nothing_else(dev, sep, fill, H, W):
    """x, the packed weights and the flat output are carved from a guarded arena: no guard byte changes, x and the weights are
    unchanged, every output element is written, and the result equals an unguarded call's bit for bit.  W = 11 and W = 1 are no
    multiple of 4."""
    tag, _, head = sep
    x = torch.from_numpy(np.random.default_rng(H * W).standard_normal((2, 64, H, W)).astype(np.float32))
    with torch.no_grad():
        plain = head(x.to(dev))
        folded = head.folded()
    arena = Arena(dev, fill, capacity=16 << 20)
    gx, gp = arena.put(x, "x"), arena.put(folded.packed, "packed")
    out = arena.out((2 * sum(folded.channels) * H * W,), torch.float32, "out")
    guarded = copy.copy(folded)
    guarded.packed = gp
    res = cm.center_heads_forward(gx, guarded, out)
    assert res is not None
    arena.check()
    assert torch.equal(gx.cpu(), x) and torch.equal(gp, folded.packed)
    base = 0
    for (name, want), got in zip(plain.items(), res[0]):
        assert got.data_ptr() == out.data_ptr() + 4 * base and torch.equal(got, want), name
        base += got.numel()
    assert base == out.numel()


# ---- task and channel edges --------------------------------------------------------------------------------------------------------
EDGES = {
    "one_head_one_channel": [dict(height=(1, 2))],
    "c16": [dict(heatmap=(16, 2), reg=(2, 2))],
    "ten_classes": [dict(reg=(2, 2), heatmap=(10, 2))],
    "eight_tasks": [dict(reg=(2, 2), heatmap=(t % 3 + 1, 2)) for t in range(8)],
}


@pytest.mark.parametrize("case", list(EDGES))
@pytest.mark.parametrize("k", [3, 1])
def test_task_and_channel_edges_against_float64(dev, case, k):
    tasks = [cm.SeparateHead(64, dict(h), final_kernel=k).eval() for h in EDGES[case]]
    for t, task in enumerate(tasks):
        load_seeded(task, 500 + t)
    x = torch.from_numpy(np.random.default_rng(len(case) + k).standard_normal((2, 64, 7, 15)).astype(np.float32))
    want = {f"{t}.{n}": v for t, task in enumerate(tasks) for n, v in float64_of(task, x).items()}
    stacks = [[(name, getattr(task.to(dev), name)) for name in task.heads] for task in tasks]
    with torch.no_grad():
        res = cm.center_heads_forward(x.to(dev), cm.fold_center_heads(stacks, k))
    assert res is not None and [len(r) for r in res] == [len(t.heads) for t in tasks]
    got = {f"{t}.{n}": v for t, (task, r) in enumerate(zip(tasks, res)) for n, v in zip(task.heads, r)}
    bar = min(bars(f"sep{k}").values())
    check(f"edges/{case}_k{k}", got, want, lambda key: bar)


# ---- fallback only where documented ------------------------------------------------------------------------------------------------
def test_module_falls_back_to_its_torch_layers_only_where_documented(dev, sep):
    tag, host, head = sep
    k = head.final_kernel
    x = torch.from_numpy(gen.inputs(tag))
    xd = x.to(dev)
    own = bars(tag)
    low = min(own.values())
    golden = {str(key): GOLD[f"{tag}.out64.{key}"] for key in GOLD[tag + ".keys"]}
    failures = []
    with torch.no_grad():
        assert head.fusable(xd)
        check(f"{tag}/fused", head(xd), golden, own.__getitem__, failures)
        head.use_fused = False
        try:
            assert not head.fusable(xd)
            check(f"{tag}/fallback_use_fused_false", head(xd), golden, own.__getitem__, failures)
        finally:
            head.use_fused = True
    assert not head.fusable(xd)                              # gradients enabled and the parameters require them
    out = head(xd)
    assert all(v.requires_grad for v in out.values())
    check(f"{tag}/fallback_gradient", out, golden, own.__getitem__, failures)
    with torch.no_grad():
        assert not head.fusable(xd.double()) and not head.fusable(x)
        # train mode: batch statistics, against a float64 copy in train mode
        trained, want = copy.deepcopy(head).train(), None
        ref = copy.deepcopy(host).train().double()
        want = ref(x.double())
        assert not trained.fusable(xd)
        check(f"{tag}/fallback_train", trained(xd), want, own.__getitem__, failures)
        variants = {
            "head_conv48": (cm.SeparateHead(64, dict(gen.SEP_HEADS), head_conv=48, final_kernel=k), low),
            "num_conv3": (cm.SeparateHead(64, dict(reg=(2, 3), heatmap=(2, 2)), final_kernel=k), 1.5 * low),
            "no_running_stats": (cm.SeparateHead(64, dict(gen.SEP_HEADS), final_kernel=k, norm_cfg=dict(type="BN2d", track_running_stats=False)),
                                 low),
        }
        for name, (module, bar) in variants.items():
            load_seeded(module, 900)
            module.eval()
            want = float64_of(module, x)
            module = module.to(dev)
            assert not module.fusable(xd), name
            check(f"{tag}/fallback_{name}", module(xd), want, lambda key, bar=bar: bar, failures)
    assert not failures, failures


# ---- CenterHead ---------------------------------------------------------------------------------------------------------------------
PC = [-4.8, -4.8, -5.0, 4.8, 4.8, 3.0]
TRAIN_CFG = dict(point_cloud_range=PC, grid_size=[gen.HEAD_MAP * 8, gen.HEAD_MAP * 8, 1], voxel_size=[0.1, 0.1, 0.2], out_size_factor=8,
                 dense_reg=1, gaussian_overlap=0.1, max_objs=20, min_radius=2, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2])
TEST_CFG = dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_per_img=500, max_pool_nms=False, min_radius=[4, 0.85],
                score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1], nms_type=["circle", "rotate"], pre_max_size=1000,
                post_max_size=83, nms_thr=0.2, nms_scale=[[1.0], [1.0, 2.5]])
BBOX_CODER = dict(type="CenterPointBBoxCoder", pc_range=PC, post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=20,
                  score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9)
LOSS_CLS = dict(type="GaussianFocalLoss", reduction="mean")
LOSS_BBOX = dict(type="L1Loss", reduction="mean", loss_weight=0.25)


def build_center_head(dev):
    head = cm.CenterHead(**gen.head_kwargs(), train_cfg=dict(TRAIN_CFG), test_cfg=dict(TEST_CFG), bbox_coder=dict(BBOX_CODER),
                         loss_cls=dict(LOSS_CLS), loss_bbox=dict(LOSS_BBOX))
    w = load_seeded(head, gen.HEAD_SEED)
    assert gen.digest(gen.inputs("head"), w) == str(GOLD["head.inputs_sha256"])
    return head.eval().to(dev)


@pytest.fixture(scope="module")
def center(dev):
    return build_center_head(dev), torch.from_numpy(gen.inputs("head")).to(dev)


def golden_head():
    return {str(k): GOLD[f"head.out64.{k}"] for k in GOLD["head.keys"]}


def test_center_head_forward_single_fused_and_unfused_meets_every_bar(center):
    head, x = center
    failures = []
    with torch.no_grad():
        assert head.fusable(x)
        check("head/fused", flat(head, x), golden_head(), bars("head").__getitem__, failures)
        head.use_fused = False
        try:
            assert not head.fusable(x) and not any(t.use_fused for t in head.task_heads)
            check("head/torch", flat(head, x), golden_head(), bars("head").__getitem__, failures)
        finally:
            head.use_fused = True
        res = head(x)
    assert isinstance(res, tuple) and len(res) == 2 and all(isinstance(r, list) and len(r) == 1 for r in res)
    assert not failures, failures


def test_center_head_forward_replays_under_a_graph(center):
    head, x = center
    rng = np.random.default_rng(11)
    fresh = lambda: x + torch.from_numpy(rng.standard_normal(tuple(x.shape)).astype(np.float32) * 1e-3).to(x.device)   # noqa: E731
    static = x.clone()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            head(static)                                      # the warm-up forward builds the fold
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                         # a capture admits no sync, no read-back and no copy from the host
            out = flat(head, static)
        for _ in range(2):
            contents = fresh()
            static.copy_(contents)
            graph.replay()
            torch.cuda.synchronize()
            eager = flat(head, contents)
            for key in eager:
                assert torch.equal(out[key], eager[key]), key


def test_center_head_forward_has_no_host_sync(center):
    head, x = center
    with torch.no_grad():
        head(x)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            head(x)
        finally:
            torch.cuda.set_sync_debug_mode("default")


def test_center_head_train_mode_backpropagates_and_updates_the_running_statistics(dev):
    head = build_center_head(dev).train()
    x = torch.from_numpy(gen.inputs("head")).to(dev)
    before = head.task_heads[1].vel[0].bn.running_mean.clone()
    assert not head.fusable(x)
    out = head.forward_single(x)
    loss = sum(v.float().square().mean() for d in out for v in d.values())
    loss.backward()
    for p in (head.shared_conv.conv.weight, head.shared_conv.bn.weight, head.task_heads[0].reg[0].conv.weight,
              head.task_heads[1].heatmap[1].bias, head.task_heads[1].vel[1].weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
    assert int(head.task_heads[1].vel[0].bn.num_batches_tracked) == 8 and int(head.shared_conv.bn.num_batches_tracked) == 8
    assert not torch.equal(head.task_heads[1].vel[0].bn.running_mean, before)


def ground_truth(dev):
    rng = np.random.default_rng(21)
    gt_boxes, gt_labels = [], []
    for n in (3, 5):
        xy = rng.uniform(-4.0, 4.0, (n, 2))
        rest = np.concatenate([rng.uniform(-1.0, 1.0, (n, 1)), rng.uniform(0.6, 2.5, (n, 3)), rng.uniform(-3.0, 3.0, (n, 1)),
                               rng.uniform(-1.0, 1.0, (n, 2))], axis=1)
        gt_boxes.append(torch.from_numpy(np.concatenate([xy, rest], axis=1).astype(np.float32)).to(dev))
        gt_labels.append(torch.from_numpy(rng.integers(0, 3, n).astype(np.int64)).to(dev))
    return gt_boxes, gt_labels


def same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def test_center_head_get_bboxes_equals_the_function(center):
    head, x = center
    with torch.no_grad():
        preds = head(x)
        got = head.get_bboxes(preds)
        want = heads.centerhead_get_bboxes(preds, head.bbox_coder, TEST_CFG, [1, 2], norm_bbox=True, sync=True)
        assert len(got) == len(want) == gen.HEAD_B
        for g, w in zip(got, want):
            assert sorted(g) == ["bboxes", "labels", "scores"] and all(torch.equal(g[key], w[key]) for key in g)
        loose = head.get_bboxes(preds, sync=False)
        want = heads.centerhead_get_bboxes(preds, head.bbox_coder, TEST_CFG, [1, 2], norm_bbox=True, sync=False)
        assert sorted(loose) == sorted(want) and all(torch.equal(loose[key], want[key]) for key in want)
        wrapped = head.get_bboxes(preds, [dict(box_type_3d=lambda t, box_dim: ("boxes", t, box_dim)) for _ in range(gen.HEAD_B)])
        for (boxes, scores, labels), g in zip(wrapped, got):
            assert boxes[0] == "boxes" and boxes[2] == 9 and torch.equal(boxes[1], g["bboxes"])
            assert torch.equal(scores, g["scores"]) and torch.equal(labels, g["labels"])


def test_center_head_get_targets_and_loss_are_the_functions_on_the_heads_own_settings(dev):
    head = build_center_head(dev)
    x = torch.from_numpy(gen.inputs("head")).to(dev)
    gt_boxes, gt_labels = ground_truth(dev)
    preds = head(x)                                           # eval mode, gradients on: the torch layers, a graph to the parameters
    targets = head.get_targets(gt_boxes, gt_labels)
    want_targets = heads.centerhead_get_targets(gt_boxes, gt_labels, [1, 2], TRAIN_CFG, norm_bbox=True)
    assert len(targets) == len(want_targets) == 4 and same(targets, want_targets)
    assert tuple(targets[0][1].shape) == (gen.HEAD_B, 2, gen.HEAD_MAP, gen.HEAD_MAP) and int(sum(m.sum() for m in targets[3])) > 0
    losses = head.loss(gt_boxes, gt_labels, preds)
    want = heads.centerhead_loss(preds, want_targets, code_weights=TRAIN_CFG["code_weights"], loss_cls=LOSS_CLS, loss_bbox=LOSS_BBOX)
    assert sorted(losses) == sorted(want) == sorted(["heatmap/task0", "bbox/task0", "heatmap/task1", "bbox/task1"])
    for key in want:
        assert torch.equal(losses[key], want[key]) and bool(torch.isfinite(losses[key]).all()), key
    # second call onwards (the first builds the cached offsets of the list form): loss and its backward raise on any host sync
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = head.loss(gt_boxes, gt_labels, preds)
        sum(again.values()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(again[key], want[key]) for key in want)
    for p in (head.shared_conv.conv.weight, head.task_heads[1].reg[0].conv.weight, head.task_heads[0].heatmap[1].bias):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
