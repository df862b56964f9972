"""GPU: pillar / radar encoder kernels against tests/golden/pillar_encoder_ref.npz (the REFERENCE's modules on CPU torch, see
tests/golden/make_pillar_encoder_golden.py) and against each other.

Bars: decorate is bit-equal to the reference except f_cluster (bound derived in tests/test_pillar_encoder.py) and, with_distance
only, the distance column (two fp32 evaluations of sqrt(x^2 + y^2 + z^2): each within 2.5 ulp of the exact value — three
products and two sums under the root, halved by it, plus the root's own rounding — so they differ by at most 6 * 2^-24 |d|).  The
fused eval stack is held to 4 x e_ref against the reference's float64 recomputation, e_ref being the reference's own
fp32-vs-float64 error; train-mode quantities to 4 x the reference's own fp32-vs-float64 error of each quantity; scatter is
bit-equal."""
import numpy as np
import pytest
import torch

from bevfusion_amd import pillar_encoder as pe, synth
from bevfusion_amd.voxel import Voxelization
from conftest import record_parity
from test_pillar_encoder import build_net, case_inputs, check_fcluster, check_train, gen, gold  # noqa: F401

pytestmark = pytest.mark.gpu


def to(dev, *tensors):
    return [t.to(dev) for t in tensors]


def assert_same_bits(got, ref, what):
    """Bit equality with a message that names the columns that differ."""
    diff = got.view(np.int32) != ref.view(np.int32)
    if diff.any():
        cols = {int(c): int(diff[..., c].sum()) for c in np.nonzero(diff.any(axis=tuple(range(diff.ndim - 1))))[0]}
        i = tuple(int(v[0]) for v in np.nonzero(diff))
        raise AssertionError(f"{what}: {int(diff.sum())} words differ, per column {cols}; first at {i}: got {got[i]!r} ({got.view(np.int32)[i]:#x}) "
                             f"want {ref[i]!r} ({ref.view(np.int32)[i]:#x})")


@pytest.mark.parametrize("case", list(gen.CASES))
def test_decorate_matches_the_reference(case, gold, dev):
    c = gen.CASES[case]
    F, P = c["in_channels"], c["P"]
    feats, num, coors = case_inputs(case, gold)
    net = build_net(case, gold).to(dev)
    before = feats.clone()
    decor = net.decorate(*to(dev, feats, num, coors)).cpu().numpy()
    assert torch.equal(feats, before)
    host = net.cpu().decorate(feats, num, coors).numpy()          # bit-equal to the reference (tests/test_pillar_encoder.py)
    if c["kind"] == "pillar":
        real = np.arange(P)[None, :] < num.numpy()[:, None]
        check_fcluster(decor[:, :, F:F + 3][real], gold[case + ".fcluster"], feats, num, P)
        assert not decor[:, :, F:F + 3][~real].any()
        decor[:, :, F:F + 3] = host[:, :, F:F + 3] = 0
        if c["with_distance"]:
            d = host[:, :, F + 5].astype(np.float64)
            assert np.all(np.abs(decor[:, :, F + 5] - d) <= 6 * 2.0 ** -24 * np.abs(d))
            decor[:, :, F + 5] = host[:, :, F + 5] = 0
    assert_same_bits(decor, host, "GPU decorate vs the host formulation")
    if not c["with_distance"]:
        assert gen.sha(decor) == str(gold[case + ".decor_sha256"]), "decorated tensor differs from the reference's bytes"


def test_radar_decorate_nan_to_num(gold, dev):
    feats, num, coors = case_inputs("radar", gold)
    bad = torch.from_numpy(gen.inject_nonfinite(feats.numpy()))
    decor = build_net("radar").to(dev).decorate(*to(dev, bad, num, coors)).cpu().numpy()
    assert_same_bits(decor, build_net("radar").decorate(bad, num, coors).numpy(), "nan_to_num case vs the host formulation")
    assert not np.isnan(decor).any() and decor[1, 0, 6] == np.finfo(np.float32).max and decor[2, 0, 7] == -np.finfo(np.float32).max
    assert gen.sha(decor) == str(gold["radar.decor_nonfinite_sha256"])


@pytest.mark.parametrize("case", list(gen.CASES))
def test_fused_eval_stack_matches_the_reference(case, gold, dev):
    feats, num, coors = to(dev, *case_inputs(case, gold))
    net = build_net(case, gold).to(dev).eval()
    ref64 = gen.unpack64(gold[case + ".eval64_hi"], gold[case + ".eval64_q"], gold[case + ".eval64_scale"])
    e_ref = float(gold[case + ".e_ref"])
    with torch.no_grad():
        assert net._fused(feats, num, coors) is not None          # the fused kernel takes this shape
        out = net(feats, num, coors)
        net.use_fused = False
        unfused = net(feats, num, coors)
    err, err_unfused = gen.rel_err(out.cpu().numpy(), ref64), gen.rel_err(unfused.cpu().numpy(), ref64)
    print(f"{case}: e_ref {e_ref:.3e}  fused {err:.3e}  unfused {err_unfused:.3e}")
    record_parity(f"pillar_encoder/{case}/reference_fp32_vs_fp64", e_ref, 4 * e_ref)
    record_parity(f"pillar_encoder/{case}/fused_vs_fp64", err, 4 * e_ref)
    record_parity(f"pillar_encoder/{case}/unfused_vs_fp64", err_unfused, 4 * e_ref)
    assert out.shape == ref64.shape and err <= 4 * e_ref
    assert err_unfused <= 4 * e_ref


def test_padded_rows_take_part_in_the_max(gold, dev):
    """One real point whose activations all lie below relu(shift): the maxima are the padded rows' values."""
    feats, num, coors = (torch.from_numpy(a) for a in gen.inputs("pillar", M=40, seed=11))
    num[:] = 1
    feats[:, 1:] = 0
    for case in ("pillar_dist", "pillar"):
        net = build_net(case).eval()
        first = net.pfn_layers[0]
        with torch.no_grad():
            x = net.decorate(feats, num, coors)[0, 0]              # pillar 0's real row
            first.norm.bias.fill_(2.0)
            first.norm.running_mean.zero_()
            first.norm.weight.copy_(-torch.sign(first.linear.weight @ x) * first.norm.weight.abs())
            net = net.to(dev)
            out = net(*to(dev, feats, num, coors))
            net.use_fused = False
            unfused = net(*to(dev, feats, num, coors))
            scale, shift = first.folded()[1:]
            act = torch.relu((first.linear.weight @ x.to(dev)) * scale + shift)
            assert bool((act < torch.relu(shift)).all())
        if case == "pillar_dist":                                  # one layer: the output IS relu(shift)
            assert torch.allclose(out[0], torch.relu(shift), rtol=1e-6, atol=0)
        assert float((out - unfused).abs().max()) <= 4 * float(gold[case + ".e_ref"]) * float(unfused.abs().max())


@pytest.mark.parametrize("case,M", [("radar", 60000), ("pillar", 30000)])
def test_fused_and_unfused_agree_at_max_voxels(case, M, gold, dev):
    # the radar grid has 2 x 128 x 128 cells: four samples hold its max_voxels distinct pillars
    feats, num, coors = to(dev, *(torch.from_numpy(a) for a in gen.inputs(case, M=M, seed=31, B=4 if case == "radar" else 2)))
    net = build_net(case).to(dev).eval()
    with torch.no_grad():
        out = net(feats, num, coors)
        net.use_fused = False
        unfused = net(feats, num, coors)
    e_ref = float(gold[case + ".e_ref"])
    err = float((out - unfused).abs().max()) / float(unfused.abs().max())
    print(f"{case} x {M}: fused vs unfused {err:.3e} (bar {4 * e_ref:.3e})")
    record_parity(f"pillar_encoder/{case}/fused_vs_unfused_{M}", err, 4 * e_ref)
    assert out.shape == (M, 64) and err <= 4 * e_ref


@pytest.mark.parametrize("case", list(gen.CASES))
def test_train_mode_matches_the_reference(case, gold, dev):
    """Decorate kernel + the module's own torch layers and autograd against the reference's CPU results; every figure is
    printed before anything is asserted.  The tightest quantity is the weight gradient of the last Linear, a reduction over all
    M x P rows: summed in blocks of 512 rows (`_RowsLinear`) it sits at 1.9e-06 (pillar, bar 6.2e-06) and 3.7e-06 (radar, bar
    1.5e-05) on an MI355X; as one long fp32 GEMM it was 1.4e-05 and 3.8e-05."""
    feats, num, coors = to(dev, *case_inputs(case, gold))
    net = build_net(case, gold).to(dev).train()
    out = net(feats, num, coors)
    (out * torch.from_numpy(gen.loss_weights(case, tuple(out.shape))).to(dev)).sum().backward()
    check_train(net, case, gold, out.detach().cpu().numpy())


def golden_canvas(name, gold):
    c = gen.SCATTER_CASES[name]
    f, co = gen.scatter_inputs(name)
    assert gen.sha(f, co) == str(gold[name + ".inputs_sha256"])
    cells, rows = gold[name + ".cells"], gold[name + ".rows"]
    ncell = c["nx"] * c["ny"]
    flat = np.zeros((c["B"], c["C"], ncell), np.float32)
    flat[cells // ncell, :, cells % ncell] = f[rows]
    assert gen.sha(flat) == str(gold[name + ".canvas_sha256"]), "the canvas does not rebuild the reference's bytes"
    return f, co, flat.reshape(c["B"], c["C"], c["nx"], c["ny"]), rows


@pytest.mark.parametrize("name", list(gen.SCATTER_CASES))
def test_scatter_matches_the_reference(name, gold, dev):
    c = gen.SCATTER_CASES[name]
    f, co, ref, rows = golden_canvas(name, gold)
    mod = pe.PointPillarsScatter(c["C"], (c["nx"], c["ny"]))
    feats = torch.from_numpy(f).to(dev).requires_grad_(True)
    coors = torch.from_numpy(co).to(dev)
    canvas = mod(feats, coors, c["B"])
    assert canvas.shape == ref.shape and np.array_equal(canvas.detach().cpu().numpy().view(np.int32), ref.view(np.int32))
    assert int((canvas.detach().abs().sum(1) > 0).sum()) == int(gold[name + ".nonzero_cells"]) == len(rows)
    canvas.backward(torch.from_numpy(gen.scatter_grad(name)).to(dev))
    grad = feats.grad.cpu().numpy()
    assert gen.sha(grad) == str(gold[name + ".grad_sha256"])
    losers = np.setdiff1d(np.arange(c["M"]), rows)
    assert not grad[losers].any() and (len(losers) > 0) == (name == "scatter128_dup")
    # fp16 rows: the fp32 golden cast to fp16
    half = mod(torch.from_numpy(f).to(dev).half(), coors, c["B"])
    assert half.dtype == torch.float16 and torch.equal(half.cpu(), torch.from_numpy(ref).half())


def test_scatter_resets_a_dirty_winner_plane(gold, dev):
    from bevfusion_amd import _capi

    name = "scatter128_dup"
    c = gen.SCATTER_CASES[name]
    f, co, ref, _ = golden_canvas(name, gold)
    feats, coors = torch.from_numpy(f).to(dev), torch.from_numpy(co).to(dev)
    winner = torch.full((c["B"], c["nx"] * c["ny"]), 7, dtype=torch.int32, device=dev)     # stale winners everywhere
    canvas = torch.full((c["B"], c["C"], c["nx"], c["ny"]), 3.0, device=dev)
    lib = _capi.load()
    for _ in range(2):
        _capi.check(lib.bevamd_pillar_scatter_forward(_capi.ptr(feats), 0, _capi.ptr(coors), c["M"], c["C"], c["B"], c["nx"], c["ny"],
                                                      _capi.ptr(winner), _capi.ptr(canvas), _capi.stream_ptr(dev)), "scatter")
        assert np.array_equal(canvas.cpu().numpy().view(np.int32), ref.view(np.int32))
    assert int((winner >= 0).sum()) == int(gold[name + ".nonzero_cells"])


def _voxelized(dev, kind, B=2):
    cfg = dict(voxel_size=[0.2, 0.2, 8] if kind == "pillar" else [0.8, 0.8, 8], point_cloud_range=gen.RANGE, max_num_points=20,
               max_voxels=(30000, 60000))
    vox = Voxelization(**cfg).eval()
    fs, cs, ns = [], [], []
    for k in range(B):
        pts = synth.lidar_points(seed=k, sweeps=1)
        pts = pts[(np.abs(pts[:, 0]) < 51.2) & (np.abs(pts[:, 1]) < 51.2) & (pts[:, 2] > -5.0) & (pts[:, 2] < 3.0)]
        if kind == "radar":                                         # rows widened to 45 columns
            extra = np.random.default_rng(100 + k).uniform(-1, 1, (pts.shape[0], 40)).astype(np.float32)
            pts = np.concatenate([pts, extra], 1)[::8]
        f, c, n = vox(torch.from_numpy(np.ascontiguousarray(pts)).to(dev))
        fs.append(f)
        cs.append(torch.nn.functional.pad(c, (1, 0), mode="constant", value=k))   # BEVFusion.voxelize
        ns.append(n)
    return torch.cat(fs), torch.cat(cs), torch.cat(ns)


@pytest.mark.parametrize("kind", ["pillar", "radar"])
def test_encoders_end_to_end_from_voxelization(kind, gold, dev):
    B = 2
    feats, coords, sizes = _voxelized(dev, kind, B)
    if kind == "pillar":
        enc = pe.PointPillarsEncoder(dict(type="PillarFeatureNet", **gen.net_kwargs("pillar")),
                                     dict(type="PointPillarsScatter", in_channels=64, output_shape=[512, 512]))
        nx = 512
    else:
        enc = pe.RadarEncoder(dict(type="RadarFeatureNet", **gen.net_kwargs("radar")),
                              dict(type="PointPillarsScatter", in_channels=64, output_shape=[128, 128]), pts_bev_encoder=None)
        nx = 128
    torch.manual_seed(0)
    for m in enc.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 1.5)
            m.bias.data.uniform_(0.05, 0.3)                         # positive shifts: every pillar leaves a non-zero cell
    enc = enc.to(dev).eval()
    assert feats.shape[1] == 20 and int(coords[:, 1:3].min()) >= 0 and int(coords[:, 1:3].max()) < nx
    with torch.no_grad():
        out = enc(feats, coords, B, sizes)
        enc.pts_voxel_encoder.use_fused = False
        ref = enc(feats, coords, B, sizes)
    assert tuple(out.shape) == (B, 64, nx, nx)
    cells = torch.unique((coords[:, 0].long() * nx + coords[:, 1]) * nx + coords[:, 2]).numel()
    assert cells == coords.shape[0] and int((out.abs().sum(1) > 0).sum()) == cells
    assert float((out - ref).abs().max()) <= 4 * float(gold[kind + ".e_ref"]) * float(ref.abs().max())
    assert torch.equal(out == 0, ref == 0)


def test_graph_capture_replays_the_eval_encoder(gold, dev):
    feats, num, coors = to(dev, *case_inputs("radar", gold))
    enc = pe.RadarEncoder(dict(type="RadarFeatureNet", **gen.net_kwargs("radar")),
                          dict(type="PointPillarsScatter", in_channels=64, output_shape=[128, 128])).to(dev).eval()
    enc.pts_voxel_encoder.load_state_dict(build_net("radar").state_dict())
    static = [torch.zeros_like(feats), torch.ones_like(num), torch.zeros_like(coors)]
    with torch.no_grad():
        ref = enc(feats, coors, 2, num).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enc(static[0], static[2], 2, static[1])                 # folded parameters are cached before the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = enc(static[0], static[2], 2, static[1])
    for s, t in zip(static, (feats, num, coors)):
        s.copy_(t)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        out.fill_(7.0)                                              # the replay writes every word again
