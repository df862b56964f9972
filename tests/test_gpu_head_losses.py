"""GPU: the head losses (csrc/ext/head_losses.hip) against tests/golden/head_losses_ref.npz and the host formulation.

Bar, everywhere (the rule of DESIGN 3.14): max(4 x the reference's own fp32-vs-float64 error, 2 ulp (fp32) of the output's largest
magnitude).  For the fixtures the reference's error is the one stored in the golden; for the edge and config shapes it is the error
of `_losses_host` in fp32 against `_losses_host` in float64.  Where the float64 gradient is exactly 0 the device's is exactly 0.
Observed errors and bars are printed and recorded (conftest.record_parity)."""
import numpy as np
import pytest
import torch

from bevfusion_amd import head_losses, heads
from conftest import record_parity
from test_head_losses import CH, TF, ch_call, gold, inputs, tf_call, total  # noqa: F401

pytestmark = pytest.mark.gpu
CODE_WEIGHTS = list(head_losses._DEFAULT_CODE_WEIGHTS)
CLS, BOX, HEAT = head_losses._CLS, head_losses._BOX, head_losses._HEAT


def ulp2(want):
    return 2 * float(np.spacing(np.float32(np.abs(np.asarray(want, np.float64)).max())))


def check(tag, got, want, ref_err):
    """`got` (device, fp32) against the float64 `want` under the bar; exact zeros where `want` is exactly 0."""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64)
    want = np.asarray(want.detach().cpu().numpy() if torch.is_tensor(want) else want, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bar = max(4 * float(ref_err), ulp2(want))
    err = float(np.abs(got - want).max())
    print(f"{tag}: error {err:.3e}, bar {bar:.3e} (reference fp32 error {float(ref_err):.3e})")
    record_parity(f"head_losses/{tag}", err, bar)
    assert err <= bar, (tag, err, bar)
    assert not got[want == 0].any(), f"{tag}: a gradient that is exactly 0 in float64 is not 0"


def maxerr(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max())


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TF) + list(CH))
def test_fixture_parity(gold, name, dev):
    if name in TF:
        losses, leaves = tf_call(gold, name, torch.float32, dev, sync_free=True)
    else:
        losses, leaves = ch_call(gold, name, torch.float32, dev)
    total(losses).backward()
    torch.cuda.synchronize()
    for k in losses:
        check(f"{name}/loss/{k}", losses[k], gold[f"{name}/loss/{k}"], gold[f"{name}/err_loss/{k}"])
    for k, leaf in leaves.items():
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape
        check(f"{name}/grad/{k}", leaf.grad, gold[f"{name}/grad/{k}"], gold[f"{name}/err_grad/{k}"])
    i = inputs(gold, name)
    maps = ["heatmap_target"] if name in TF else [f"heatmap_target{t}" for t in range(CH[name])]
    preds = ["dense_heatmap"] if name in TF else [f"heatmap{t}" for t in range(CH[name])]
    _, num_pos = head_losses.gaussian_focal_forward([torch.from_numpy(i[p]).to(dev) for p in preds], [torch.from_numpy(i[m]).to(dev) for m in maps])
    want = [gold[f"{name}/num_pos/heat"]] if name in TF else [gold[f"{name}/num_pos/heat{t}"] for t in range(CH[name])]
    assert num_pos.cpu().tolist() == [float(w) for w in want]


# ---- the dense kernels at their edge shapes ---------------------------------------------------------------------------------------------
def dense_case(sizes, seed):
    """Seeded (logits, targets) per map on the host; some targets exactly 1, some logits clamped."""
    g = torch.Generator().manual_seed(seed)
    xs, ts = [], []
    for n in sizes:
        x = (torch.randn(n, generator=g) * 2.5).clamp_(-9, 9)                    # clear of the clamp edge at +-log(9999)
        t = torch.rand(n, generator=g) ** 3 * 0.9
        t[torch.randperm(n, generator=g)[:max(1, n // 50)]] = 1.0
        x[torch.randperm(n, generator=g)[:n // 40]] = 12.0
        xs.append(x)
        ts.append(t)
    return xs, ts


def dense_reference(xs, ts, weights, dtype, device):
    """sum_t weights[t] * loss[t] and its gradients by the host formulation.  -> (losses [T], grads)."""
    leaves = [x.to(device=device, dtype=dtype).requires_grad_(True) for x in xs]
    losses = []
    for x, t in zip(leaves, ts):
        t = t.to(device=device, dtype=dtype)
        avg = torch.clamp(t.eq(1).to(dtype).sum(), min=1)
        losses.append(head_losses._gaussian_focal_host(head_losses._clip_sigmoid(x), t).sum() / avg)
    losses = torch.stack(losses)
    (losses * weights.to(device=device, dtype=dtype)).sum().backward()
    return losses.detach(), [x.grad for x in leaves]


def dense_check(tag, xs, ts, dev, place_pred=None, place_target=None, place_grad=None):
    """The device's forward and backward for the maps against the host formulation; place_*(i, tensor): where map i lies."""
    to_dev = lambda i, v: v.to(dev)   # noqa: E731
    T = len(xs)
    weights = torch.linspace(0.5, 1.5, T)
    px = [(place_pred or to_dev)(i, x) for i, x in enumerate(xs)]
    pt = [(place_target or to_dev)(i, t) for i, t in enumerate(ts)]
    loss, num_pos = head_losses.gaussian_focal_forward(px, pt)
    out = None if place_grad is None else [place_grad(i, torch.zeros_like(x)) for i, x in enumerate(xs)]
    grads = head_losses.gaussian_focal_backward(px, pt, num_pos, weights.to(dev), out=out)
    torch.cuda.synchronize()
    l64, g64 = dense_reference(xs, ts, weights, torch.float64, dev)
    l32, g32 = dense_reference(xs, ts, weights, torch.float32, dev)
    assert num_pos.cpu().tolist() == [float((t == 1).sum()) for t in ts]
    check(f"{tag}/loss", loss, l64, maxerr(l32, l64))
    for i in range(T):
        check(f"{tag}/grad{i}", grads[i], g64[i], maxerr(g32[i], g64[i]))


def test_dense_edge_sizes(dev):
    groups, share = head_losses.head_loss_plan(2 ** 31)
    xs, ts = dense_case([1, share - 1, share, share + 1], 11)
    dense_check("edge_sizes", xs, ts, dev)
    loop = groups * share + 5                                                    # more cells than the grid covers in one pass
    assert head_losses.head_loss_plan(loop)[0] == groups
    xs, ts = dense_case([loop], 12)
    dense_check("loop_path", xs, ts, dev)


def shifted(v, floats, dev):
    """`v` on the device, its base `floats` floats past a 16-byte boundary."""
    buf = torch.zeros(v.numel() + 4, device=dev)
    view = buf[floats:floats + v.numel()]
    view.copy_(v)
    assert view.data_ptr() % 16 == 4 * floats
    return view


@pytest.mark.parametrize("shift", [(1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 0), (1, 3, 2)])
def test_dense_bases_off_the_16_byte_boundary(shift, dev):
    """Prediction, target and gradient bases 1, 2 and 3 floats past a 16-byte boundary (a scalar head, then 16-byte accesses); the
    heads' own case, only the target off the boundary; and all three different (the backward's scalar path)."""
    share = head_losses.head_loss_plan(1)[1]
    xs, ts = dense_case([share + 7, 13], 13)
    dense_check("offset_%d_%d_%d" % shift, xs, ts, dev, *[lambda i, v, s=s: shifted(v, s, dev) for s in shift])


def test_sixteen_maps_in_one_call(dev):
    xs, ts = dense_case([37 + 5 * t for t in range(16)], 14)
    flat = torch.cat(ts).to(dev)                                                 # the targets: views into one buffer, as the head's are
    starts = np.concatenate([[0], np.cumsum([t.numel() for t in ts])])
    dense_check("sixteen_maps", xs, ts, dev, None, lambda i, v: flat[starts[i]:starts[i + 1]])
    with pytest.raises(ValueError):
        head_losses.gaussian_focal_forward([x.to(dev) for x in xs] + [xs[0].to(dev)], [t.to(dev) for t in ts] + [ts[0].to(dev)])


# ---- whole heads at seeded shapes ---------------------------------------------------------------------------------------------------------
def tf_case(B, C, S, L, K, D, seed, empty=False):
    g = torch.Generator().manual_seed(seed)
    P = L * K
    xs, ts = dense_case([B * C * S * S], seed + 1)
    preds = {"dense_heatmap": xs[0].view(B, C, S, S), "heatmap": torch.randn(B, C, P, generator=g) * 1.5}
    if empty:
        ts[0][ts[0] == 1] = 0.5
    for n, w in zip(head_losses.PIECES[:5 if D == 10 else 4], (2, 1, 3, 2, 2)):
        preds[n] = torch.randn(B, w, P, generator=g)
    labels = torch.full((B, P), C, dtype=torch.int64)
    if not empty:
        pos = torch.rand(B, P, generator=g) < 0.2
        labels[pos] = torch.randint(0, C, (int(pos.sum()),), generator=g)
    weights = (torch.rand(B, P, generator=g) > 0.1).to(torch.int64)
    live = (labels < C)[..., None]
    targets = (labels, weights, torch.randn(B, P, D, generator=g) * live, live.expand(B, P, D).float().contiguous(), None,
               int(live.sum()), 0.25, ts[0].view(B, C, S, S))
    return preds, targets


def tf_run(preds, targets, K, C, L, dtype, dev, host):
    leaves = {n: v.to(device=dev, dtype=dtype).requires_grad_(True) for n, v in preds.items()}
    tg = tuple(t.to(dev) if torch.is_tensor(t) else t for t in targets)
    D = targets[2].shape[2]
    if host:
        losses = head_losses._losses_host("transfusion", leaves, tg, K, C, L, CODE_WEIGHTS[:D], CLS, BOX, HEAT)
    else:
        losses = heads.transfusion_loss(leaves, tg, K, C, L)
    total(losses).backward()
    return losses, leaves


def tf_compare(tag, preds, targets, K, C, L, dev):
    got, got_leaves = tf_run(preds, targets, K, C, L, torch.float32, dev, host=False)
    l64, g64 = tf_run(preds, targets, K, C, L, torch.float64, dev, host=True)
    l32, g32 = tf_run(preds, targets, K, C, L, torch.float32, dev, host=True)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(l64)
    for k in got:
        check(f"{tag}/loss/{k}", got[k], l64[k], maxerr(l32[k], l64[k]))
    for k in got_leaves:
        check(f"{tag}/grad/{k}", got_leaves[k].grad, g64[k].grad, maxerr(g32[k].grad, g64[k].grad))
    return got, got_leaves


def ch_case(B, classes, S, M, seed, live, same_cell=None):
    g = torch.Generator().manual_seed(seed)
    preds, heat, anno, inds, masks = [], [], [], [], []
    for t, c in enumerate(classes):
        xs, ts = dense_case([B * c * S * S], seed + 10 * t)
        d = {"heatmap": xs[0].view(B, c, S, S)}
        for n, w in zip(head_losses.CH_PIECES, (2, 1, 3, 2, 2)):
            d[n] = torch.randn(B, w, S, S, generator=g)
        preds.append(d)
        heat.append(ts[0].view(B, c, S, S))
        ind = torch.zeros(B, M, dtype=torch.int64)
        mask = torch.zeros(B, M, dtype=torch.uint8)
        n = live[t]
        for b in range(B):
            ind[b, :n] = torch.randint(0, S * S, (n,), generator=g) if same_cell is None else same_cell
            mask[b, :n] = 1
        anno.append(torch.randn(B, M, 10, generator=g) * mask[..., None])
        inds.append(ind)
        masks.append(mask)
    return preds, (heat, anno, inds, masks)


def ch_run(preds, targets, dtype, dev, host):
    leaves = [{n: v.to(device=dev, dtype=dtype).requires_grad_(True) for n, v in d.items()} for d in preds]
    tg = tuple([t.to(dev) for t in part] for part in targets)
    if host:
        losses = head_losses._losses_host("centerhead", leaves, tg, CODE_WEIGHTS, HEAT, BOX)
    else:
        losses = heads.centerhead_loss([[d] for d in leaves], tg)
    finite = [v for v in losses.values() if bool(torch.isfinite(v))]
    sum(finite).backward()
    return losses, {f"{n}{t}": v for t, d in enumerate(leaves) for n, v in d.items()}


def ch_compare(tag, preds, targets, dev, nan_tasks=()):
    got, got_leaves = ch_run(preds, targets, torch.float32, dev, host=False)
    l64, g64 = ch_run(preds, targets, torch.float64, dev, host=True)
    l32, g32 = ch_run(preds, targets, torch.float32, dev, host=True)
    torch.cuda.synchronize()
    for k in got:
        if any(k == f"bbox/task{t}" for t in nan_tasks):
            assert bool(torch.isnan(got[k])) and bool(torch.isnan(l64[k])), k     # NaN on both sides
            continue
        check(f"{tag}/loss/{k}", got[k], l64[k], maxerr(l32[k], l64[k]))
    for k, leaf in got_leaves.items():
        if g64[k].grad is None:
            continue
        check(f"{tag}/grad/{k}", leaf.grad, g64[k].grad, maxerr(g32[k].grad, g64[k].grad))
    return got


def test_one_proposal_per_layer(dev):
    preds, targets = tf_case(8, 3, 7, 2, 1, 10, 21)
    assert targets[5] > 0
    tf_compare("k1", preds, targets, 1, 3, 2, dev)


def test_a_thousand_slots_on_one_cell(dev):
    preds, targets = ch_case(1, (2,), 13, 1024, 31, live=(1024,), same_cell=5)
    ch_compare("m1024", preds, targets, dev)


def test_nan_target_gives_nan_on_both_sides(dev):
    preds, targets = ch_case(2, (1, 2), 13, 9, 32, live=(4, 3))
    targets[1][0][0, 1, 2] = float("nan")
    ch_compare("nan_target", preds, targets, dev, nan_tasks=(0,))


def test_config_shapes(dev):
    """2 x 10 x 180 x 180 with 200 proposals in one layer, and six CenterHead tasks at 180 x 180 with max_objs 500; twice: bit-equal."""
    preds, targets = tf_case(2, 10, 180, 1, 200, 10, 41)
    got, leaves = tf_compare("config/transfusion", preds, targets, 200, 10, 1, dev)
    again, leaves2 = tf_run(preds, targets, 200, 10, 1, torch.float32, dev, host=False)
    assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got)
    assert all(torch.equal(leaves[k].grad.view(torch.int32), leaves2[k].grad.view(torch.int32)) for k in leaves)
    cpreds, ctargets = ch_case(2, (1, 2, 2, 1, 2, 2), 180, 500, 42, live=(40, 25, 0, 7, 60, 3))
    cgot = ch_compare("config/centerhead", cpreds, ctargets, dev)
    cagain, cleaves2 = ch_run(cpreds, ctargets, torch.float32, dev, host=False)
    cfirst, cleaves = ch_run(cpreds, ctargets, torch.float32, dev, host=False)
    assert all(torch.equal(cgot[k].view(torch.int32), cagain[k].view(torch.int32)) for k in cgot)
    assert all(torch.equal(cleaves[k].grad.view(torch.int32), cleaves2[k].grad.view(torch.int32)) for k in cleaves)
    assert float(cgot["bbox/task2"].detach()) == 0.0


def test_loss_modules_on_the_device(dev):
    g = torch.Generator().manual_seed(51)
    p = (torch.rand(2, 3, 9, 9, generator=g) * 0.98 + 0.01)
    t = torch.rand(2, 3, 9, 9, generator=g)
    t[0, 0, 0, :3] = 1
    x, y, w = torch.randn(11, 4, generator=g), torch.randint(0, 5, (11,), generator=g), torch.randint(0, 3, (11,), generator=g)
    a, b, wb = torch.randn(2, 5, 8, generator=g), torch.randn(2, 5, 8, generator=g), torch.rand(2, 5, 8, generator=g)
    cases = [("gaussian", heads.GaussianFocalLoss(loss_weight=0.5), (p, t), dict(avg_factor=3.0)),
             ("gaussian_sum", heads.GaussianFocalLoss(reduction="sum"), (p, t), {}),
             ("focal", heads.FocalLoss(), (x, y, w), dict(avg_factor=4)),
             ("focal_mean", heads.FocalLoss(gamma=1.5), (x, y), {}),
             ("l1", heads.L1Loss(loss_weight=0.25), (a, b, wb), dict(avg_factor=torch.tensor(2.0)))]
    for tag, module, args, kw in cases:
        def run(dtype, device):
            first = args[0].clone().to(device=device, dtype=dtype).requires_grad_(True)
            rest = [v.to(device) if not v.is_floating_point() else v.to(device=device, dtype=dtype) for v in args[1:]]
            out = module(first, *rest, **kw)
            out.backward()
            return out, first.grad
        got, ggot = run(torch.float32, dev)
        l64, g64 = run(torch.float64, "cpu")
        l32, g32 = run(torch.float32, "cpu")
        check(f"module/{tag}/loss", got, l64, maxerr(l32, l64))
        check(f"module/{tag}/grad", ggot, g64, maxerr(g32, g64))
    with pytest.raises(RuntimeError, match="float32"):
        heads.GaussianFocalLoss()(p.to(dev).half(), t.to(dev).half())


# ---- no sync, graphs -----------------------------------------------------------------------------------------------------------------------
def test_no_host_sync_from_targets_to_backward(dev):
    """transfusion_get_targets(sync=False) -> transfusion_loss -> backward, warmed, with every synchronising call an error."""
    from test_gpu_head_assign import device_inputs, gen, make_assigner, make_coder

    case = "layers"
    c = gen.CASES[case]
    coder, assigner, cfg = make_coder(case), make_assigner(case), gen.case_cfg(case)
    preds, gt, kw = device_inputs(case, dev, "packed")
    size = cfg["grid_size"][0] // cfg["out_size_factor"]
    preds = {k: v.clone().requires_grad_(True) for k, v in preds.items()}
    preds["dense_heatmap"] = torch.randn(c["B"], gen.C, size, size, device=dev).requires_grad_(True)
    plain = {k: v.detach() for k, v in preds.items()}

    def step():
        targets = heads.transfusion_get_targets(*gt, plain, coder, assigner, cfg, c["K"], gen.C, num_decoder_layers=c["L"], sync=False, **kw)
        losses = heads.transfusion_loss(preds, targets, c["K"], gen.C, c["L"], code_weights=CODE_WEIGHTS[:8])
        total(losses).backward()
        return losses, targets

    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses, targets = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(targets[5]) > 0 and all(bool(torch.isfinite(v)) for v in losses.values())
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in preds.values())
    assert float(losses["matched_ious"]) == float(targets[6])


def bits(t):
    return t.contiguous().view(torch.int32)


def test_graph_replay_over_fresh_contents(dev):
    """The op functions captured under no_grad, warmed on a side stream; three contents with other positive counts (one with none)
    go through the same buffers: every replay is bit-equal to the eager call on those buffers."""
    B, C, S, L, K, D = 2, 3, 11, 2, 5, 10
    classes, M = (1, 2), 9
    contents = [(tf_case(B, C, S, L, K, D, 61), ch_case(B, classes, S, M, 71, live=(4, 2))),
                (tf_case(B, C, S, L, K, D, 62, empty=True), ch_case(B, classes, S, M, 72, live=(0, 0))),
                (tf_case(B, C, S, L, K, D, 63), ch_case(B, classes, S, M, 73, live=(9, 1)))]
    assert len({c[0][1][5] for c in contents}) == 3 and contents[1][0][1][5] == 0

    def flatten(content):
        (preds, tg), (cpreds, ctg) = content
        out = [preds[n] for n in ("dense_heatmap", "heatmap") + head_losses.PIECES] + [tg[0], tg[1], tg[2], tg[3], tg[7],
                                                                                     torch.tensor(tg[5], dtype=torch.int32)]
        for d in cpreds:
            out += [d[n] for n in ("heatmap",) + head_losses.CH_PIECES]
        for part in ctg:
            out += list(part)
        return out

    static = [v.to(dev).clone() for v in flatten(contents[0])]
    g_tf = torch.linspace(0.5, 1.5, 1 + 2 * L, device=dev)
    g_ch = torch.linspace(0.7, 1.3, 2 * len(classes), device=dev)

    def step():
        dense, scores, *rest = static
        pieces, (labels, weights, btargets, bweights, heat, num_pos) = rest[:5], rest[5:11]
        ch = rest[11:]
        T = len(classes)
        heat_preds = [ch[6 * t] for t in range(T)]
        maps = [ch[6 * t + 1:6 * t + 6] for t in range(T)]
        heatmaps, anno, inds, masks = (ch[6 * T + T * j:6 * T + T * (j + 1)] for j in range(4))
        with torch.no_grad():
            losses, heat_pos = head_losses.transfusion_loss_forward(dense, heat, scores, labels, weights, pieces, btargets, bweights, num_pos, L)
            gd, gs, gp = head_losses.transfusion_loss_backward(dense, heat, scores, labels, weights, pieces, btargets, bweights, num_pos,
                                                               heat_pos, g_tf, L)
            closses, cpos, avg = head_losses.centerhead_loss_forward(heat_preds, heatmaps, maps, inds, anno, masks)
            gh, gm = head_losses.centerhead_loss_backward(heat_preds, heatmaps, maps, inds, anno, masks, cpos, avg, g_ch)
        return [losses, heat_pos, gd, gs] + list(gp) + [closses, cpos, avg] + list(gh) + [g for task in gm for g in task]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    seen = []
    for content in (contents[1], contents[2], contents[0]):
        for buf, v in zip(static, flatten(content)):
            buf.copy_(v.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in out]
        eager = step()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(replayed, eager))
        seen.append((float(replayed[1]), float(replayed[0][0])))
    assert seen[0][0] == 0 and len({s[1] for s in seen}) == 3                     # fresh contents, fresh results
