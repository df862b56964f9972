"""CPU: CenterHead / SeparateHead as modules — registry and config building, state-dict names and shapes, the torch path against
tests/golden/centerhead_module_ref.npz (outputs of the REFERENCE's SeparateHead and CenterHead.forward_single exec'd single-threaded
on CPU torch by tests/golden/make_centerhead_module_golden.py; inputs and weights are regenerated here from the seeds and checked
against the stored SHA-256), the fold and its cache, the packed weight order, the argument checks of the new entry point, the
binding table and the resources of the new kernel's code object.

Tolerance of an output: per head, max |got - float64| / max |float64| <= 4 x e_ref, e_ref being the reference's own fp32 deviation
from its float64 recomputation, normalised the same way.  The factor covers another order of the 576-term sums and the BatchNorm
folded into a scale and a shift."""
import copy
import ctypes
import importlib.util
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import test_kernel_resources as resources
from bevfusion_amd import _capi, centerhead_module as cm, heads
from bevfusion_amd.config import load_config
from bevfusion_amd.registry import HEADS
from conftest import record_parity

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "centerhead_module_ref.npz")
REF_CONFIGS = "/root/reference/configs"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="the reference's configs are not present")
BAR_FACTOR = 4.0

_spec = importlib.util.spec_from_file_location("make_centerhead_module_golden", os.path.join(HERE, "golden", "make_centerhead_module_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def recorded_shapes(gold, tag):
    return [(str(n), tuple(int(d) for d in str(s).split(",")) if str(s) else ()) for n, s in zip(gold[tag + ".names"], gold[tag + ".shapes"])]


def build(gold, tag):
    """Our module for a recording, loaded with the seeded state (strict), in eval mode."""
    if tag == "head":
        module = cm.CenterHead(**gen.head_kwargs())
    else:
        module = cm.SeparateHead(64, dict(gen.SEP_HEADS), final_kernel=gen.SEP[tag]["final_kernel"])
    shapes = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    assert shapes == recorded_shapes(gold, tag)
    w = gen.weights(shapes, gen.seed_of(tag))
    assert gen.digest(gen.inputs(tag), w) == str(gold[tag + ".inputs_sha256"]), "inputs and weights do not rebuild the fixture's bytes"
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    return module.eval()


def run(module, x):
    """{key: tensor} with the golden's keys."""
    if isinstance(module, cm.CenterHead):
        return {f"{t}.{name}": v for t, d in enumerate(module.forward_single(x)) for name, v in d.items()}
    return module(x)


def deviation(got, ref64):
    return float(np.abs(np.asarray(got, np.float64) - ref64).max() / np.abs(ref64).max())


def bars(gold, tag):
    """key -> (e_ref, bar)."""
    out = {}
    for key in gold[tag + ".keys"]:
        e_ref = deviation(gold[f"{tag}.out32.{key}"], gold[f"{tag}.out64.{key}"])
        out[str(key)] = (e_ref, BAR_FACTOR * e_ref)
    return out


# ---- registry and config -----------------------------------------------------------------------------------------------------------
def check_full_size_head(head):
    assert isinstance(head, cm.CenterHead) and head.num_classes == [1, 2, 2, 1, 2, 2] and len(head.task_heads) == 6
    assert head.shared_conv.conv.in_channels == 256 and head.shared_conv.conv.out_channels == 64 and head.shared_conv.conv.bias is None
    for task, classes in zip(head.task_heads, head.num_classes):
        assert isinstance(task, cm.SeparateHead) and task.final_kernel == 3 and task.in_channels == 64
        assert list(task.heads) == ["reg", "height", "dim", "rot", "vel", "heatmap"]
        assert [task.heads[k][0] for k in task.heads] == [2, 1, 3, 2, 2, classes]
        assert task.heatmap[0].conv.kernel_size == (3, 3) and task.heatmap[1].padding == (1, 1)
    assert isinstance(head.bbox_coder, heads.CenterPointBBoxCoder)
    assert isinstance(head.loss_cls, heads.GaussianFocalLoss) and isinstance(head.loss_bbox, heads.L1Loss)
    assert head.norm_bbox is True and head.train_cfg["code_weights"][-1] == 0.2 and head.use_fused in (True, False)
    assert head._foldable() is False                                   # a fresh module is in train mode
    assert head.eval()._foldable() is True


def test_the_heads_are_registered_and_reexported():
    assert HEADS.get("CenterHead") is cm.CenterHead and HEADS.get("SeparateHead") is cm.SeparateHead
    assert heads.CenterHead is cm.CenterHead and heads.SeparateHead is cm.SeparateHead
    assert heads.center_heads_forward is cm.center_heads_forward and heads.HEADS is HEADS


def test_dcn_separate_head_is_not_registered():
    with pytest.raises(KeyError, match="DCNSeparateHead"):
        HEADS.build(dict(type="DCNSeparateHead", in_channels=64, num_cls=1, heads=dict(), dcn_config=dict()))
    with pytest.raises(KeyError, match="DCNSeparateHead"):
        cm.CenterHead(in_channels=32, tasks=[["a"]], separate_head=dict(type="DCNSeparateHead", dcn_config=dict()))


def test_the_recorded_yaml_config_builds_the_head_and_is_left_unchanged(gold):
    cfg = json.loads(str(gold["yaml.head_cfg"]))
    assert cfg["type"] == "CenterHead"
    before = copy.deepcopy(cfg)
    check_full_size_head(HEADS.build(cfg))
    assert cfg == before


def test_the_constructor_leaves_the_callers_dicts_alone():
    separate = dict(type="SeparateHead", init_bias=-2.19, final_kernel=3)
    common = dict(reg=(2, 2), height=(1, 2))
    head = cm.CenterHead(in_channels=16, tasks=[["a"], ["b", "c"]], common_heads=common, separate_head=separate)
    assert separate == dict(type="SeparateHead", init_bias=-2.19, final_kernel=3)      # the reference adds in_channels, heads, num_cls
    assert common == dict(reg=(2, 2), height=(1, 2))
    assert [list(t.heads) for t in head.task_heads] == [["reg", "height", "heatmap"]] * 2
    assert [t.heads["heatmap"] for t in head.task_heads] == [(1, 2), (2, 2)]


@needs_ref
def test_the_reference_yaml_chain_builds_the_head(gold):
    cfg = load_config(os.path.join(REF_CONFIGS, str(gold["yaml.leaf"])))["model"]["heads"]["object"]
    assert json.dumps(cfg) == str(gold["yaml.head_cfg"])
    check_full_size_head(HEADS.build(cfg))


@pytest.mark.parametrize("tag", ["sep3", "sep1", "head"])
def test_state_dict_names_and_shapes_equal_the_reference(gold, tag):
    build(gold, tag)                             # asserts the list and loads with strict=True
    names = [n for n, _ in recorded_shapes(gold, tag)]
    prefix = "task_heads.1." if tag == "head" else ""
    for want in ("reg.0.conv.weight", "reg.0.bn.running_var", "reg.0.bn.num_batches_tracked", "heatmap.1.weight", "heatmap.1.bias"):
        assert prefix + want in names
    assert prefix + "reg.0.conv.bias" not in names
    if tag == "head":
        assert "shared_conv.conv.weight" in names and "shared_conv.bn.running_mean" in names and "shared_conv.conv.bias" not in names


# ---- the torch path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["sep3", "sep1", "head"])
def test_torch_path_on_host_tensors_against_the_float64_reference(gold, tag):
    module = build(gold, tag)
    x = torch.from_numpy(gen.inputs(tag))
    assert not module.fusable(x)                 # host tensors: the torch layers
    with torch.no_grad():
        got = run(module, x)
    assert list(got) == [str(k) for k in gold[tag + ".keys"]]
    observed = {}
    for key, (e_ref, bar) in bars(gold, tag).items():
        assert tuple(got[key].shape) == gold[f"{tag}.out64.{key}"].shape
        err = deviation(got[key].numpy(), gold[f"{tag}.out64.{key}"])
        observed[key] = dict(reference=e_ref, observed=err, bar=bar)
        record_parity(f"centerhead_module/{tag}/torch_cpu/{key}_reference", e_ref, bar)     # the reference's own deviation ...
        record_parity(f"centerhead_module/{tag}/torch_cpu/{key}", err, bar)                 # ... next to what this path gives
        print(f"{tag} torch path {key}: reference {e_ref:.3e}, observed {err:.3e}, bar {bar:.3e}")
    for key, o in observed.items():
        assert o["observed"] <= o["bar"], (key, o)


def test_forward_returns_the_multi_apply_shape_on_the_cpu(gold):
    head = build(gold, "head")
    x = torch.from_numpy(gen.inputs("head"))
    with torch.no_grad():
        res = head(x)
        two = head([x, x[:1]])
        single = head.forward_single(x)
    assert isinstance(res, tuple) and len(res) == 2 and all(isinstance(r, list) and len(r) == 1 for r in res)
    assert all(torch.equal(res[t][0][k], single[t][k]) for t in range(2) for k in single[t])
    assert len(two) == 2 and all(len(r) == 2 for r in two) and two[1][1]["heatmap"].shape == (1, 2, gen.HEAD_MAP, gen.HEAD_MAP)


def test_init_weights_sets_the_heatmap_bias_and_moves_the_fold():
    head = cm.SeparateHead(64, dict(reg=(2, 2), heatmap=(3, 2)), final_kernel=3).eval()
    first = head.folded()
    assert head.folded() is first                # equal versions: the cached fold
    old = head.reg[0].conv.weight.detach().clone()
    head.init_weights()
    assert bool((head.heatmap[-1].bias.detach() == torch.tensor(-2.19)).all())
    assert bool((head.reg[-1].bias.detach() == 0).all()) and not torch.equal(head.reg[0].conv.weight.detach(), old)
    assert head.folded() is not first            # written under no_grad, not through .data: the versions moved
    center = cm.CenterHead(in_channels=8, tasks=[["a"], ["b"]], common_heads=dict(reg=(2, 2)))
    center.init_weights()
    assert all(float(t.heatmap[-1].bias.detach()[0]) == pytest.approx(-2.19) for t in center.task_heads)


# ---- the fold ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["sep3", "sep1"])
def test_fold_against_a_float64_formula_and_the_packed_order(gold, tag):
    head = build(gold, tag)
    k = head.final_kernel
    folded = head.folded()
    assert folded.final_kernel == k and folded.heads_per_task == [6] and folded.channels == [2, 1, 3, 2, 2, 2]
    assert folded.names == [list(gen.SEP_HEADS)] and folded.packed.dtype == torch.float32 and folded.packed.data_ptr() % 16 == 0
    state = {n: v.double() for n, v in head.state_dict().items()}
    offset = 0
    for i, name in enumerate(gen.SEP_HEADS):
        scale = state[f"{name}.0.bn.weight"] / torch.sqrt(state[f"{name}.0.bn.running_var"] + 1e-5)
        shift = state[f"{name}.0.bn.bias"] - state[f"{name}.0.bn.running_mean"] * scale
        assert float((folded.scales[i].double() - scale).abs().max()) <= 2.0 ** -22 * float(scale.abs().max())
        assert float((folded.shifts[i].double() - shift).abs().max()) <= 2.0 ** -21 * float(shift.abs().max() + 1)
        # a host-side unpack of the block gives the module's weights back bit for bit
        assert folded.offsets[i] == offset
        c = folded.channels[i]
        n1 = 4096 * k * k
        block = folded.packed[offset:]
        assert torch.equal(cm.center_heads_unpack_w1(block[:n1], k), getattr(head, name)[0].conv.weight.detach())
        assert torch.equal(block[n1:n1 + 64], folded.scales[i]) and torch.equal(block[n1 + 64:n1 + 128], folded.shifts[i])
        w2 = block[n1 + 128:n1 + 128 + c * k * k * 64].view(c, k, k, 64).permute(0, 3, 1, 2)
        assert torch.equal(w2, getattr(head, name)[1].weight.detach())
        bias = block[n1 + 128 + c * k * k * 64:][:(c + 3) // 4 * 4]
        assert torch.equal(bias[:c], getattr(head, name)[1].bias.detach()) and bool((bias[c:] == 0).all())
        offset += n1 + 128 + c * k * k * 64 + (c + 3) // 4 * 4
    assert folded.packed.numel() == offset


def test_packed_order_names_the_fragment_element():
    """Element [m][s4][lane][q] of the packed first convolution, spelled out for a few lanes and steps."""
    for k in (1, 3):
        w = torch.arange(64 * 64 * k * k, dtype=torch.float32).view(64, 64, k, k)
        flat = cm.center_heads_pack_w1(w).view(2, 8 * k * k, 64, 4)
        for m, s4, lane, q in ((0, 0, 0, 0), (1, 0, 33, 3), (0, 8 * k * k - 1, 63, 2), (1, 5 * k * k, 17, 1)):
            kk = 2 * (4 * s4 + q) + (lane >> 5)
            tap, ci = divmod(kk, 64)
            assert float(flat[m, s4, lane, q]) == float(w[m * 32 + (lane & 31), ci, tap // k, tap % k])
        assert torch.equal(cm.center_heads_unpack_w1(flat.reshape(-1), k), w)


def test_fold_cache_is_reused_on_equal_versions_and_rebuilt_after_an_in_place_write(gold):
    head = build(gold, "head")
    first = head.folded()
    assert head.folded() is first and len(first.channels) == 12 and first.heads_per_task == [6, 6]
    with torch.no_grad():
        head.task_heads[1].vel[0].bn.running_mean.add_(1.0)
    second = head.folded()
    assert second is not first and not torch.equal(second.shifts[10], first.shifts[10]) and torch.equal(second.shifts[9], first.shifts[9])
    head.load_state_dict(head.state_dict())
    assert head.folded() is not second


def test_fusable_reads_the_module_state(gold):
    head = build(gold, "sep3")
    assert head._foldable()
    assert not head.train()._foldable()          # batch statistics
    assert head.eval()._foldable()
    assert not cm.SeparateHead(64, dict(reg=(2, 3)), final_kernel=3).eval()._foldable()          # num_conv != 2
    assert not cm.SeparateHead(64, dict(reg=(2, 2)), head_conv=48, final_kernel=3).eval()._foldable()
    assert not cm.SeparateHead(32, dict(reg=(2, 2)), final_kernel=3).eval()._foldable()
    assert not cm.SeparateHead(64, dict(heatmap=(17, 2)), final_kernel=3).eval()._foldable()
    assert not cm.SeparateHead(64, dict(reg=(2, 2)), final_kernel=5).eval()._foldable()
    assert not cm.SeparateHead(64, dict(reg=(2, 2)), final_kernel=3, norm_cfg=dict(type="BN2d", track_running_stats=False)).eval()._foldable()
    assert not cm.SeparateHead(64, {f"h{i}": (1, 2) for i in range(9)}, final_kernel=1).eval()._foldable()
    nine = cm.CenterHead(in_channels=8, tasks=[["a"]] * 9, common_heads=dict(reg=(2, 2))).eval()
    assert not nine._foldable()
    with pytest.raises(RuntimeError, match="needs GPU tensors"):
        cm.center_heads_forward(torch.zeros(1, 64, 2, 2), head.folded())


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def _block(k, c):
    return 4096 * k * k + 128 + c * k * k * 64 + (c + 3) // 4 * 4


def _call(lib, batch=2, channels=64, head_conv=64, H=9, W=11, k=3, per_task=(2,), chans=(2, 1), x=1, packed=1, out=1, tables=True,
          packed_floats=None, out_floats=None):
    """bevamd_center_heads_forward with made-up non-null addresses: every case here is refused before any GPU work."""
    if packed_floats is None:
        packed_floats = sum(_block(k, c) for c in chans)
    if out_floats is None:
        out_floats = batch * sum(chans) * H * W
    addr = lambda on: ctypes.c_void_p(on * 4096 or None)   # noqa: E731
    return lib.bevamd_center_heads_forward(addr(x), batch, channels, head_conv, H, W, k, len(per_task), _capi.ints(per_task) if tables else None,
                                           _capi.ints(chans) if tables else None, addr(packed), packed_floats, addr(out), out_floats, None)


@pytest.mark.parametrize("kwargs, code, word", [
    (dict(channels=48), 4, "must be 64"),
    (dict(head_conv=48), 4, "must be 64"),
    (dict(k=5), 4, "1 or 3"),
    (dict(k=2), 4, "1 or 3"),
    (dict(per_task=(1,) * 9, chans=(1,) * 9), 4, "1 .. 8"),
    (dict(per_task=(), chans=()), 4, "1 .. 8"),
    (dict(per_task=(9,), chans=(1,) * 9), 4, "9 heads, 1 .. 8"),
    (dict(per_task=(0, 2), chans=(2, 1)), 4, "0 heads, 1 .. 8"),
    (dict(chans=(2, 17)), 4, "17 channels, 1 .. 16"),
    (dict(chans=(0, 1)), 4, "0 channels, 1 .. 16"),
    (dict(H=0), 1, "bad sizes"),
    (dict(W=-3), 1, "bad sizes"),
    (dict(batch=-1), 1, "batch"),
    (dict(batch=65536), 1, "batch"),
    (dict(tables=False), 1, "null host array"),
    (dict(packed_floats=7), 1, "packed holds 7 floats"),
    (dict(out_floats=5), 1, "out holds 5 floats"),
    (dict(packed=0), 1, "packed is null"),
    (dict(x=0), 1, "x or out is null"),
    (dict(out=0), 1, "x or out is null"),
])
def test_entry_point_refuses_before_any_gpu_work(kwargs, code, word):
    lib = _capi.load()
    assert _call(lib, **kwargs) == code and word in _capi.last_error(), _capi.last_error()


def test_an_empty_batch_is_nothing_to_do():
    assert _call(_capi.load(), batch=0, x=0, out=0) == 0


def test_binding_table_equals_the_header():
    txt = open(os.path.join(ROOT, "include", "bevfusion_amd_ext.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(bevamd_center_heads_\w+)\s*\(([^)]*)\)", txt)}
    assert sorted(protos) == ["bevamd_center_heads_forward"]
    args = protos["bevamd_center_heads_forward"].split(",")
    res, argtypes = _capi._EXT_SIGNATURES["bevamd_center_heads_forward"]
    want = [ctypes.c_void_p if "*" in a else ctypes.c_longlong if "long long" in a else ctypes.c_int for a in args]
    assert res is ctypes.c_int and argtypes == want
    assert "size_t" not in protos["bevamd_center_heads_forward"]       # no workspace, no sized buffer
    assert "bevamd_center_heads_forward" in _capi.ext_exported_names()


# ---- the code object ---------------------------------------------------------------------------------------------------------------
def _lds_bytes(obj):
    """kernel (demangled, up to the argument list) -> group_segment_fixed_size of one in-tree object's gfx950 code object."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fb, co = os.path.join(tmp, "x.fb"), os.path.join(tmp, "x.co")
        subprocess.run([resources.TOOLS[0], f"--dump-section=.hip_fatbin={fb}", obj], check=True, capture_output=True)
        subprocess.run([resources.TOOLS[1], "--unbundle", "--type=o", f"--input={fb}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--output={co}"], check=True, capture_output=True)
        notes = subprocess.run([resources.TOOLS[2], "--notes", co], capture_output=True, text=True, check=True).stdout
    for blk in notes.split("    .args:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk)
        if name and lds:
            dem = subprocess.run(["c++filt", name.group(1)], capture_output=True, text=True).stdout.strip()
            out[re.sub(r"\(.*", "", dem)] = int(lds.group(1))
    return out


@pytest.mark.skipif(not os.path.exists(os.path.join(resources.OBJ, "center_heads.o")) or not all(os.path.exists(t) for t in resources.TOOLS),
                    reason="needs the in-tree objects of bevfusion_amd.build and the ROCm llvm tools")
def test_the_new_kernels_use_no_scratch_spill_nothing_and_fit_two_workgroups_of_lds():
    kernels = {n: v for n, v in resources._kernels().items() if v["obj"] == "center_heads"}
    names = ["void bevamd::center_heads_kernel<1>", "void bevamd::center_heads_kernel<3>"]
    assert sorted(kernels) == names
    lds = _lds_bytes(os.path.join(resources.OBJ, "center_heads.o"))
    for name in names:
        got = kernels[name]
        assert got["scratch"] == 0 and got["vgpr_spills"] == 0, (name, got)
        assert got["regs"] <= 256, (name, got)                          # two workgroups of four waves per compute unit
        assert 0 < lds[name] <= 160 * 1024, (name, lds[name])
        assert 2 * lds[name] <= 160 * 1024, (name, lds[name])           # ... and by LDS as well
