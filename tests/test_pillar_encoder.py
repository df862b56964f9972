"""CPU: pillar / radar encoders — C ABI, registry, module trees, config building, argument validation, and the host-tensor path
against tests/golden/pillar_encoder_ref.npz (outputs of the REFERENCE's PillarFeatureNet / RadarFeatureNet / PointPillarsScatter
exec'd single-threaded on CPU torch by tests/golden/make_pillar_encoder_golden.py; inputs and weights are regenerated here from
the seed and checked against the stored SHA-256).

Tolerances: an eval output is held to 4 x e_ref against the reference's own float64 recomputation, e_ref being the reference's
fp32-vs-float64 error from the fixture (both normalised by max |float64 output|); a train-mode quantity is held to 4 x the
reference's own fp32-vs-float64 error of that quantity against the recorded fp32 value.  f_cluster is a sum of <= P fp32 terms in
a free order plus one division: |got - ref| <= 2 (P - 1) 2^-24 max_p |x_p| + 2^-23 |mean|."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi, pillar_encoder as pe
from bevfusion_amd.config import build_hot_path, load_config
from bevfusion_amd.registry import BACKBONES

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "pillar_encoder_ref.npz")
REF_CONFIGS = "/root/reference/configs"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="/root/reference not present (GPU box)")

_spec = importlib.util.spec_from_file_location("make_pillar_encoder_golden",
                                               os.path.join(HERE, "golden", "make_pillar_encoder_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def build_net(case, gold=None):
    """Our module for a fixture case, loaded with the seeded state."""
    c = gen.CASES[case]
    cls = pe.PillarFeatureNet if c["kind"] == "pillar" else pe.RadarFeatureNet
    net = cls(**gen.net_kwargs(case))
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    st = gen.state(shapes, c["seed"])
    if gold is not None:
        assert gen.sha(*st.values()) == str(gold[case + ".state_sha256"]), "weights do not rebuild the fixture's bytes"
    net.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return net


def case_inputs(case, gold):
    f, n, co = gen.inputs(case)
    assert gen.sha(f, n, co) == str(gold[case + ".inputs_sha256"]), "inputs do not rebuild the fixture's bytes"
    return torch.from_numpy(f), torch.from_numpy(n), torch.from_numpy(co)


def check_fcluster(got, ref, feats, num, P):
    """got / ref [sum(num), 3] (real rows); feats [M, P, F]."""
    x = feats[:, :, :3].double().numpy()
    bound_pillar = 2 * (P - 1) * 2.0 ** -24 * np.abs(x).max(1) + 2.0 ** -23 * np.abs(x.sum(1) / num.numpy()[:, None])   # [M, 3]
    bound = np.repeat(bound_pillar, num.numpy(), axis=0)
    assert got.shape == ref.shape == bound.shape
    assert np.all(np.abs(got.astype(np.float64) - ref) <= bound), float(np.max(np.abs(got - ref) - bound))


def check_decor(decor, case, gold, feats, num, key="decor_sha256"):
    c = gen.CASES[case]
    F, P = c["in_channels"], c["P"]
    decor = decor.copy()
    if c["kind"] == "pillar":
        real = np.arange(P)[None, :] < num.numpy()[:, None]
        check_fcluster(decor[:, :, F:F + 3][real], gold[case + ".fcluster"], feats, num, P)
        assert not decor[:, :, F:F + 3][~real].any()
        decor[:, :, F:F + 3] = 0
    assert gen.sha(decor) == str(gold[case + "." + key]), "decorated tensor differs from the reference's bytes"


def check_train(net, case, gold, out, scale=4.0):
    """Every figure is printed (observed error and bar, both relative to max |reference|) before anything is asserted."""
    p = case + "."
    tol = lambda ref, err: scale * float(err) * float(np.max(np.abs(ref)))   # noqa: E731
    sd, params = net.state_dict(), dict(net.named_parameters())
    figures = [("train_out", out, gold[p + "train_out"], gold[p + "train_out_err"])]
    figures += [(k, sd[k[len(p + "train_stat."):]].detach().cpu().numpy(), gold[k], gold[k.replace("train_stat.", "train_stat_err.")])
                for k in gold.files if k.startswith(p + "train_stat.") and "tracked" not in k]
    figures += [(k, params[k[len(p + "train_grad."):]].grad.detach().cpu().numpy(), gold[k], gold[k.replace("train_grad.", "train_grad_err.")])
                for k in gold.files if k.startswith(p + "train_grad.")]
    for name, got, ref, err in figures:
        print(f"{case} {name}: observed {np.max(np.abs(got - ref)) / np.max(np.abs(ref)):.3e}  bar {scale * float(err):.3e}")
    ref = gold[p + "train_out"]
    assert np.max(np.abs(out - ref)) <= tol(ref, gold[p + "train_out_err"])
    sd = net.state_dict()
    stats = [k[len(p + "train_stat."):] for k in gold.files if k.startswith(p + "train_stat.")]
    assert stats and len(stats) == 3 * len(gen.CASES[case]["feat_channels"])
    for k in stats:
        ref, got = gold[p + "train_stat." + k], sd[k].detach().cpu().numpy()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == 4
        else:
            assert np.max(np.abs(got - ref)) <= tol(ref, gold[p + "train_stat_err." + k]), k
    params = dict(net.named_parameters())
    grads = [k[len(p + "train_grad."):] for k in gold.files if k.startswith(p + "train_grad.")]
    assert sorted(grads) == sorted(params)
    for k in grads:
        ref, got = gold[p + "train_grad." + k], params[k].grad.detach().cpu().numpy()
        assert np.max(np.abs(got - ref)) <= tol(ref, gold[p + "train_grad_err." + k]), k


# ---- C ABI, registry, trees ---------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    names = ["bevamd_pillar_decorate", "bevamd_pillar_stack_forward", "bevamd_pillar_scatter_forward", "bevamd_pillar_scatter_backward"]
    header = open(os.path.join(os.path.dirname(HERE), "include", "bevfusion_amd_ext.h")).read()
    ext = ctypes.CDLL(_capi.EXT_LIB_PATH)
    main = os.popen(f"nm -D --defined-only {_capi.LIB_PATH}").read()
    for n in names:
        assert n + "(" in header and n in _capi.ext_exported_names() and hasattr(ext, n) and f" {n}\n" not in main
    assert _capi.load().bevamd_pillar_decorate is not None


def test_registry_names_resolve():
    for n in ("PillarFeatureNet", "RadarFeatureNet", "PointPillarsScatter", "PointPillarsEncoder", "RadarEncoder"):
        assert n in BACKBONES and BACKBONES.get(n) is getattr(pe, n)
    enc = BACKBONES.build(dict(type="RadarEncoder", pts_voxel_encoder=dict(type="RadarFeatureNet", in_channels=45, feat_channels=[64]),
                               pts_middle_encoder=dict(type="PointPillarsScatter", in_channels=64, output_shape=[128, 128]),
                               pts_bev_encoder=None))
    assert enc.pts_bev_encoder is None and enc.post_scatter is None and enc.pts_transformer_encoder is None
    with pytest.raises(KeyError):
        pe.RadarEncoder(dict(type="RadarFeatureNet"), dict(type="PointPillarsScatter"), pts_bev_encoder=dict(type="NoSuchBackbone"))


def test_state_dict_keys_match_the_reference(gold):
    for case in gen.CASES:
        net = build_net(case, gold)
        assert list(net.state_dict()) == json.loads(str(gold[case + ".state_keys"]))
    net = pe.PillarFeatureNet(5, [64, 64])
    assert net.pfn_layers[0].units == 32 and net.pfn_layers[0].linear.in_features == 10 and net.pfn_layers[1].linear.in_features == 64
    bn = net.pfn_layers[0].norm
    assert isinstance(bn, torch.nn.BatchNorm1d) and bn.eps == 1e-3 and bn.momentum == 0.01
    mask = pe.get_paddings_indicator(torch.tensor([3, 1]), 4)
    assert mask.tolist() == [[True, True, True, False], [True, False, False, False]]


@needs_ref
def test_reference_configs_build_the_encoders():
    hp = build_hot_path(load_config(REF_CONFIGS + "/nuscenes/det/transfusion/secfpn/lidar/pointpillars.yaml"))
    enc = hp["lidar_backbone"]
    assert isinstance(enc, pe.PointPillarsEncoder) and isinstance(enc.pts_voxel_encoder, pe.PillarFeatureNet)
    lin = [(l.linear.in_features, l.linear.out_features) for l in enc.pts_voxel_encoder.pfn_layers]
    assert lin == [(10, 32), (64, 64)]
    assert isinstance(enc.pts_middle_encoder, pe.PointPillarsScatter) and (enc.pts_middle_encoder.nx, enc.pts_middle_encoder.ny) == (512, 512)
    assert hp["voxelize"].max_num_points == 20 and hp["voxelize_reduce"] is False

    # camera+radar/default.yaml is a base file: its camera view transform is only completed by resnet50/default.yaml below it
    # (in_channels, out_channels, feature_size), so the whole hot path is built from that leaf and the radar part from both
    base = load_config(REF_CONFIGS + "/nuscenes/det/centerhead/lssfpn/camera+radar/default.yaml")
    leaf = load_config(REF_CONFIGS + "/nuscenes/det/centerhead/lssfpn/camera+radar/resnet50/default.yaml")
    assert base["model"]["encoders"]["radar"] == leaf["model"]["encoders"]["radar"] and not leaf["model"]["encoders"].get("lidar")
    from bevfusion_amd.vtransforms import LSSTransform

    assert sorted(build_hot_path(dict(model=dict(encoders=dict(radar=base["model"]["encoders"]["radar"]))))) == [
        "radar_backbone", "radar_voxelize", "radar_voxelize_reduce"]
    hp = build_hot_path(leaf)
    assert isinstance(hp["vtransform"], LSSTransform)
    enc = hp["radar_backbone"]
    assert isinstance(enc, pe.RadarEncoder) and isinstance(enc.pts_voxel_encoder, pe.RadarFeatureNet)
    lin = [(l.linear.in_features, l.linear.out_features) for l in enc.pts_voxel_encoder.rfn_layers]
    assert lin == [(47, 128), (128, 128), (128, 128), (128, 64)]
    assert (enc.pts_middle_encoder.nx, enc.pts_middle_encoder.ny) == (128, 128) and enc.pts_bev_encoder is None
    assert hp["radar_voxelize"].max_num_points == 20 and hp["radar_voxelize"].max_voxels == (30000, 60000)
    assert hp["radar_voxelize_reduce"] is False and "lidar_backbone" not in hp


def test_flagship_config_still_builds_the_same_modules():
    from bevfusion_amd.sparse_encoder import SparseEncoder
    from bevfusion_amd.vtransforms import DepthLSSTransform, LSSTransform

    with open(os.path.join(HERE, "golden", "host_mirror_configs.json")) as fh:
        cfgs = json.load(fh)
    hp = build_hot_path(cfgs["flagship"])
    assert sorted(hp) == ["lidar_backbone", "voxelize", "voxelize_reduce", "vtransform"]
    assert isinstance(hp["vtransform"], DepthLSSTransform) and hp["vtransform"].D == 118
    assert isinstance(hp["lidar_backbone"], SparseEncoder) and list(hp["lidar_backbone"].sparse_shape) == [1440, 1440, 41]
    assert hp["voxelize"].max_voxels == (120000, 160000)
    assert isinstance(build_hot_path(cfgs["camera_lss"])["vtransform"], LSSTransform)


# ---- host tensors against the golden ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(gen.CASES))
def test_host_forward_matches_the_reference(case, gold):
    torch.manual_seed(0)
    feats, num, coors = case_inputs(case, gold)
    net = build_net(case, gold).eval()
    before = feats.clone()
    check_decor(net.decorate(feats, num, coors).numpy(), case, gold, feats, num)
    with torch.no_grad():
        out = net(feats, num, coors)
    assert torch.equal(feats, before), "the caller's features were overwritten"
    ref64 = gen.unpack64(gold[case + ".eval64_hi"], gold[case + ".eval64_q"], gold[case + ".eval64_scale"])
    assert out.shape == ref64.shape
    assert gen.rel_err(out.numpy(), ref64) <= 4 * float(gold[case + ".e_ref"])

    net.train()
    out = net(feats, num, coors)
    (out * torch.from_numpy(gen.loss_weights(case, tuple(out.shape)))).sum().backward()
    check_train(net, case, gold, out.detach().numpy())


def test_host_radar_nan_to_num(gold):
    feats, num, coors = case_inputs("radar", gold)
    bad = torch.from_numpy(gen.inject_nonfinite(feats.numpy()))
    decor = build_net("radar").decorate(bad, num, coors).numpy()
    assert gen.sha(decor) == str(gold["radar.decor_nonfinite_sha256"])


def test_documented_differences_from_the_reference():
    feats, num, coors = (torch.from_numpy(a) for a in gen.inputs("pillar", M=1, seed=7))
    net = build_net("pillar").eval()
    with torch.no_grad():
        assert tuple(net(feats, num, coors).shape) == (1, 64)          # the reference's bare squeeze() gives [64]
    with pytest.raises(RuntimeError, match="requires_grad"):
        net(feats.clone().requires_grad_(True), num, coors)


@pytest.mark.parametrize("name", list(gen.SCATTER_CASES))
def test_host_scatter_matches_the_reference(name, gold):
    torch.set_num_threads(1)
    c = gen.SCATTER_CASES[name]
    f, co = gen.scatter_inputs(name)
    assert gen.sha(f, co) == str(gold[name + ".inputs_sha256"])
    cells, rows = gen.scatter_winners(name)
    assert np.array_equal(cells, gold[name + ".cells"]) and np.array_equal(rows, gold[name + ".rows"])
    mod = pe.PointPillarsScatter(c["C"], (c["nx"], c["ny"]))
    canvas = mod(torch.from_numpy(f), torch.from_numpy(co), c["B"])
    assert tuple(canvas.shape) == (c["B"], c["C"], c["nx"], c["ny"])
    assert gen.sha(canvas.numpy()) == str(gold[name + ".canvas_sha256"])
    assert "output_shape=(%d, %d)" % (c["nx"], c["ny"]) in repr(mod)


# ---- argument validation: no GPU needed ----------------------------------------------------------------------------------------
def test_arguments_are_validated_before_any_gpu_work():
    lib = _capi.load()
    geom = _capi.floats([0.2, 0.2, -51.1, -51.1, -51.2, -51.2, -5, 102.4, 102.4, 8])
    assert lib.bevamd_pillar_decorate(None, None, None, 10, 20, 5, 0, 0, geom, None, None) == 1
    assert "null buffer" in _capi.last_error()
    assert lib.bevamd_pillar_decorate(None, None, None, 10, 20, 5, 2, 0, geom, None, None) == 1 and "mode" in _capi.last_error()
    assert lib.bevamd_pillar_decorate(None, None, None, 10, 20, 5, 0, 0, None, None, None) == 1 and "geom" in _capi.last_error()

    def stack(P=20, F=5, mode=0, units=(32, 64), M=10, null_params=False):
        n = len(units)
        fake = (ctypes.c_void_p * n)(*[None if null_params else 256] * n)     # never dereferenced: every call below is rejected
        return lib.bevamd_pillar_stack_forward(None, None, None, M, P, F, mode, 0, geom, n, _capi.ints(units), fake, fake, fake, None, None)

    assert stack() == 1 and "null buffer" in _capi.last_error()               # supported shape, null device buffers
    assert stack(null_params=True) == 1 and "null parameter" in _capi.last_error()
    assert lib.bevamd_pillar_stack_forward(None, None, None, 10, 20, 5, 0, 0, geom, 2, None, None, None, None, None, None) == 1
    assert stack(P=33) == 4 and "not supported" in _capi.last_error()         # more than 32 rows per pillar
    assert stack(units=(32, 256)) == 4 and "not supported" in _capi.last_error()   # a width above 128
    assert stack(units=(128, 64)) == 4                                        # PFNLayer concat: 2 x 128 inputs for the next layer
    assert stack(mode=1, units=(128, 128, 128, 64), F=45) == 1                # the radar shape is supported (null buffers)
    assert stack(mode=1, units=(64, 64, 64, 64, 64)) == 4                     # more than 4 layers
    assert stack(F=65) == 4 and stack(units=(30, 64)) == 4                    # input width above 64; a width that is not a multiple of 4
    assert stack(M=0) == 0                                                    # nothing to do

    assert lib.bevamd_pillar_scatter_forward(None, 0, None, 10, 64, 2, 128, 128, None, None, None) == 1
    assert "null buffer" in _capi.last_error()
    assert lib.bevamd_pillar_scatter_forward(None, 3, None, 10, 64, 2, 128, 128, None, None, None) == 1 and "dtype" in _capi.last_error()
    assert lib.bevamd_pillar_scatter_backward(None, 0, None, None, 10, 64, 2, 128, 128, None, None) == 1
    assert lib.bevamd_pillar_scatter_backward(None, 0, None, None, 0, 64, 2, 128, 128, None, None) == 0


def test_gpu_entry_points_refuse_host_tensors():
    feats, num, coors = (torch.from_numpy(a) for a in gen.inputs("pillar", M=4, seed=1))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        pe.pillar_decorate(feats, num, coors, build_net("pillar"))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        pe.pillar_scatter(torch.zeros(4, 64), coors, 2, 512, 512)
