"""The kernels only a training step runs (spconv/fused_train.py: _Layer / _LevelConv), layer by layer against the float64 oracle
(oracle.get_indice_pairs + indice_conv + indice_conv_backward on the operands rounded to the compute type): slab forward, input
gradient on the same kernel through the mirrored transposed filter image, staged-rows filter gradient of the SubM layers, the
stem's padded 5 -> 16 path, and the strided layers (tiled forward, input gradient over the transposed table, staged-rows filter
gradient over metadata built from the layer's table) — fp16 and bf16, at every variant the training path selects between one and
eight frames per step, on small synthetic grids (partial last block, ranges walked in pieces, isolated voxels, an odd last plane).

Bars, all |err| <= bar * (1 + max|ref|): forward and input gradient the bar of test_gpu_spconv_slab.py (TOL: 1e-3 fp16, 8e-3
bf16: fp32 accumulation, one rounding of the result); filter gradient the bar of test_gpu_wgrad_slab.py (2e-3 fp16, 1.6e-2 bf16).
Every measured error goes to the parity record.

Second half: the strided filter gradient where a range can outgrow the metadata's 16-bit slots — the grid the guard keeps on the
gather kernel, the densest grid it admits, and the seam between two samples that the step's read-back catches
(fused_train.strided_wgrad_route; the bound itself: tests/test_strided_slab_bound.py)."""
import numpy as np
import pytest
import torch

import oracle
from bevfusion_amd.spconv import conv as spconv_conv
from bevfusion_amd.spconv import fused, fused_train, ops
from conftest import record_parity
from test_gpu_spconv_slab import TOL as FWD_BAR                     # forward / input gradient: the slab kernels' own bar
from test_gpu_wgrad_slab import _sorted_indices

pytestmark = pytest.mark.gpu

WG_BAR = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}              # test_gpu_wgrad_slab.py
DTYPES = [torch.float16, torch.bfloat16]
HINTS = [1.0, 2.0, 4.0, 8.0]            # either side of _SLAB_SMALL_BATCH_BELOW (1.5, 2.5) and of the 5.5 cut of fused._variant_for
_RAN = {}                               # (kernel, cin, cout, frames_hint) -> variant codes that ran
_ORACLE = {}                            # (layer, dtype, grid) -> operands and float64 results, computed once


def _name(dtype):
    return str(dtype).split(".")[-1]


def _grid(name):
    """(indices [n, 4] int32 in ascending linear index, B, shape)"""
    if name == "g40":                   # 5000 rows: a partial last block for 64-, 128- and 256-row blocks
        return _sorted_indices(np.random.default_rng(40), 2, (40, 24, 9), 2500), 2, (40, 24, 9)
    if name == "g41":                   # the strided layers: an odd X extent, so the last output plane reads two input planes
        return _sorted_indices(np.random.default_rng(41), 2, (41, 24, 9), 2500), 2, (41, 24, 9)
    if name == "tall":                  # 90 % of 96-cell lines: ranges of ~300 rows, longer than a stage
        return _sorted_indices(np.random.default_rng(5), 1, (5, 16, 96), 6900), 1, (5, 16, 96)
    shape = (40, 40, 20)
    n = {"one": 1, "isolated": 129}[name]
    lin = np.sort(np.random.default_rng(3).choice(np.arange(0, 40 * 40 * 20, 97), size=n, replace=False))
    return np.concatenate([np.zeros((n, 1), np.int64), np.stack(np.unravel_index(lin, shape), 1)], 1).astype(np.int32), 1, shape


def _case(dev, cin, cout, dtype, grid, subm, data=None):
    """Operands (rounded to `dtype`) and the oracle's float64 forward, input gradient and filter gradient of one layer on one grid
    (`grid`: a name of _grid, or any name with data = (indices, B, shape))."""
    key = (cin, cout, dtype, grid, subm)
    if key in _ORACLE:
        return _ORACLE[key]
    indices, B, shape = _grid(grid) if data is None else data
    rng = np.random.default_rng(1000 * cin + cout + (7 if dtype == torch.bfloat16 else 0))
    stride = (1, 1, 1) if subm else (2, 2, 2)
    oi, pairs, num, _ = oracle.get_indice_pairs(indices, B, shape, (3, 3, 3), stride, (1, 1, 1), (1, 1, 1), int(subm), order="cuda")
    n, m = indices.shape[0], oi.shape[0]
    x = torch.from_numpy((rng.standard_normal((n, cin)) * 0.5).astype(np.float32)).to(dtype)
    gy = torch.from_numpy((rng.standard_normal((m, cout)) * 0.5).astype(np.float32)).to(dtype)
    w = torch.from_numpy((rng.standard_normal((3, 3, 3, cin, cout)) / np.sqrt(cin * 27 / 4)).astype(np.float32))   # the fp32 master
    xf, gf, wf = x.float().numpy(), gy.float().numpy(), w.to(dtype).float().numpy()
    y_ref = oracle.indice_conv(xf, wf, pairs, num, m)
    dx_ref, dw_ref = oracle.indice_conv_backward(xf, wf, gf, pairs, num)
    c = dict(indices=indices, B=B, shape=list(shape), n=n, m=m, out_indices=oi, x=x.to(dev), gy=gy.to(dev), w=w.to(dev),
             y_ref=y_ref, dx_ref=dx_ref, dw_ref=dw_ref, pairs_off_centre=int(num.sum() - num[13]))
    _ORACLE[key] = c
    return c


@pytest.fixture(autouse=True)
def ran(monkeypatch):
    """What the layer under test launched: (kernel, cin, cout, variant) of every forward-kernel call, and the filter-gradient calls."""
    calls = []

    def spy(name, fn):
        def wrapped(*a, **kw):
            calls.append((name, a[-2], a[-1], kw.get("variant", 0)))
            return fn(*a, **kw)
        monkeypatch.setattr(ops, "sparse_conv_" + {"slab": "slab", "tiled": "tiled", "wgrad": "wgrad_slab"}[name], wrapped)

    # positional tails: sparse_conv_slab(features, image, meta, num_out, cin, cout); sparse_conv_tiled(..., num_out, K, cin, cout);
    # sparse_conv_wgrad_slab(features, out_grad, meta, cin, cout)
    spy("slab", ops.sparse_conv_slab)
    spy("tiled", ops.sparse_conv_tiled)
    spy("wgrad", ops.sparse_conv_wgrad_slab)
    return calls


def _note(ran, hint):
    for name, a, b, variant in ran:
        if name != "wgrad":
            _RAN.setdefault((name, a, b, hint), set()).add(variant)


def _err(got, ref):
    got = got.detach().float().cpu().numpy().astype(np.float64)
    return float(np.max(np.abs(got - ref))) / (1.0 + float(np.max(np.abs(ref)))) if ref.size else 0.0


def _check(tag, got, ref, bar):
    err = _err(got, ref)
    record_parity(tag, err, bar)
    print(f"{tag}: {err:.3e} (bar {bar:.1e})")
    return err <= bar, f"{tag}: {err:.3e} > {bar:.1e}"


def _layer(dev, c, conv, dtype, hint, allow_slab=True, stem_needs_grad=True, subm=True):
    """The level, plan and layer of one convolution over case `c`, driven as the encoder's walker drives them."""
    coors = torch.from_numpy(c["indices"]).to(dev)
    lvl = fused.Level(coors, c["n"], None, c["B"], c["shape"], linear_order=True, allow_slab=allow_slab)
    lvl.frames_hint = hint
    plan = fused_train._Plan(None, fused_train._Lv(lvl, c["n"]), dtype, [conv])
    L = fused_train._Layer(conv, plan, plan.lv1, plan.lv1 if subm else None)
    L.issue()
    plan.layers.append(L)
    fused_train.prepare_images(plan, dev, stem_needs_grad=stem_needs_grad)
    if not subm:
        L.lv_out = fused_train._Lv(lvl.downsample(conv.kernel_size, conv.stride, conv.padding, wait=False, want_nbr=True)[0])
        plan.pending.append(L.lv_out)
    return lvl, plan, L


def _conv(dev, c, cin, cout, subm):
    if subm:
        conv = spconv_conv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="t").to(dev)
    else:
        conv = spconv_conv.SparseConv3d(cin, cout, 3, stride=2, padding=1, bias=False, indice_key="d").to(dev)
    with torch.no_grad():
        conv.weight.copy_(c["w"])
    return conv


def _three_backwards(y, gy, conv, xr):
    """dx of the first pass, dW of three passes over the same graph"""
    dws, dx = [], None
    for i in range(3):
        conv.weight.grad = None
        if xr is not None:
            xr.grad = None
        y.backward(gy, retain_graph=i < 2)
        dws.append(conv.weight.grad.clone())
        if i == 0 and xr is not None:
            dx = xr.grad.clone()
    return dx, dws


def _run_subm(dev, ran, c, cc, dtype, hint, tag, slab=True):
    conv = _conv(dev, c, cc, cc, True)
    lvl, plan, L = _layer(dev, c, conv, dtype, hint, allow_slab=slab)
    if slab:      # the slab kernels, not the fallbacks, produce what is compared
        assert L.variant is not None and L.wg_code, (L.variant, L.wg_code)
    else:
        assert L.variant is None and L.wg_code == 0
    xr = c["x"].clone().requires_grad_(True)
    y = fused_train._LevelConv.apply(xr, conv.weight, L)
    dx, dws = _three_backwards(y, c["gy"], conv, xr)
    assert fused.geometry_status(lvl) == 0
    fwd = [r for r in ran if r[0] != "wgrad"]
    if slab:
        assert [r[0] for r in fwd] == ["slab"] * 4 and {r[3] for r in fwd} == {L.variant}, fwd      # forward + three input gradients
        assert len([r for r in ran if r[0] == "wgrad"]) == 3
    else:
        assert {r[0] for r in fwd} == {"tiled"} and not [r for r in ran if r[0] == "wgrad"]
    _note(ran, hint)
    assert dws[0].dtype == torch.float32 and tuple(dws[0].shape) == (3, 3, 3, cc, cc)
    assert torch.equal(dws[0], dws[1]) and torch.equal(dws[0], dws[2])                    # fixed-order partials, no atomics
    results = [_check(f"train {tag} forward", y, c["y_ref"], FWD_BAR[dtype]),
               _check(f"train {tag} dx", dx, c["dx_ref"], FWD_BAR[dtype]),
               _check(f"train {tag} dW", dws[0], c["dw_ref"], WG_BAR[dtype])]
    assert all(ok for ok, _ in results), [msg for ok, msg in results if not ok]
    return L


@pytest.mark.parametrize("hint", HINTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("cc", [16, 32, 64, 128])
def test_subm_layer_vs_oracle(dev, ran, cc, dtype, hint):
    """c -> c on B = 2, (40, 24, 9), 2500 cells per sample: slab forward, mirrored-image input gradient, staged-rows filter gradient."""
    c = _case(dev, cc, cc, dtype, "g40", True)
    _run_subm(dev, ran, c, cc, dtype, hint, f"subm {cc} {_name(dtype)} g40 hint {hint:g}")


@pytest.mark.parametrize("hint", [1.0, 4.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("cc", [32, 64])
def test_subm_layer_ranges_walked_in_pieces(dev, ran, cc, dtype, hint):
    """B = 1, (5, 16, 96) at 90 %: the range of a block through a kernel plane is longer than the staged rows."""
    c = _case(dev, cc, cc, dtype, "tall", True)
    L = _run_subm(dev, ran, c, cc, dtype, hint, f"subm {cc} {_name(dtype)} tall hint {hint:g}")
    meta = L.lv_in.level.subm_slab(L.wg_code)
    nblk = (c["n"] + 127) // 128
    cnt = (meta.hdr[:nblk * 24].view(torch.int32).view(nblk, 3, 2)[:, :, 1] & 0x3FFFFFFF).cpu().numpy()
    assert cnt.max() > 256, "the case must exercise the piece loop"


@pytest.mark.parametrize("hint", [1.0, 4.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("grid", ["one", "isolated"])
def test_subm_layer_tiny_sets(dev, ran, grid, dtype, hint):
    """One voxel; 129 voxels none of which has a neighbour (only the centre tap reads a row; a second block of one row)."""
    c = _case(dev, 32, 32, dtype, grid, True)
    assert c["pairs_off_centre"] == 0
    _run_subm(dev, ran, c, 32, dtype, hint, f"subm 32 {_name(dtype)} {grid} hint {hint:g}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("cc", [32, 64, 128])
def test_subm_layer_on_the_gather_kernels_of_a_batched_step(dev, ran, cc, dtype):
    """A level that may not use the slab kernels (allow_slab = False: what an overflowing range falls back to), eight frames: the
    tiled kernel's batched variant forward, the mirrored image over the layer's table backward, spconv_wgrad16 for the filter."""
    c = _case(dev, cc, cc, dtype, "g40", True)
    _run_subm(dev, ran, c, cc, dtype, 8.0, f"subm {cc} {_name(dtype)} g40 gather hint 8", slab=False)


def _match_rows(level_indices, oracle_indices, B, shape_out):
    """Row of the oracle's output set that holds the same cell as each row of the level's (no order assumed)."""
    def key(a):
        a = np.asarray(a, np.int64)
        return ((a[:, 0] * shape_out[0] + a[:, 1]) * shape_out[1] + a[:, 2]) * shape_out[2] + a[:, 3]
    ko, kl = key(oracle_indices), key(level_indices)
    order = np.argsort(ko, kind="stable")
    pos = np.searchsorted(ko[order], kl)
    assert len(np.unique(kl)) == len(kl) == len(ko) and np.array_equal(ko[order][np.minimum(pos, len(ko) - 1)], kl), "the two output sets differ"
    return order[pos]


def _run_strided(dev, ran, c, cin, cout, dtype, hint, tag, expect=None):
    """expect: None = the staged-rows filter gradient runs; "gather" = the guard keeps it off; "caught" = the read-back turns it off."""
    conv = _conv(dev, c, cin, cout, False)
    lvl, plan, L = _layer(dev, c, conv, dtype, hint, subm=False)
    if expect == "gather":
        assert L.wg_code == 0
    else:
        assert L.wg_code, "the staged-rows filter gradient serves this layer"
    xr = c["x"].clone().requires_grad_(True)
    y = fused_train._LevelConv.apply(xr, conv.weight, L)
    m = c["m"]
    assert L.lv_out.n == m and tuple(y.shape) == (m, cout)
    rows = _match_rows(L.lv_out.level.indices[:m].cpu().numpy(), c["out_indices"], c["B"], L.lv_out.level.shape)
    rows_t = torch.from_numpy(rows).to(dev)
    gy = c["gy"][rows_t].contiguous()                      # the oracle's out_grad, in the level's row order
    if expect == "caught":
        assert L.wg_checked and L.wg_code == 0, "the read-back saw the overflow of this step's metadata"
    dx, dws = _three_backwards(y, gy, conv, xr)
    wg = len([r for r in ran if r[0] == "wgrad"])
    if expect is None:
        assert fused.geometry_status(lvl) == 0 and wg == 3
    else:
        assert wg == 0
    _note(ran, hint)
    assert torch.equal(dws[0], dws[1]) and torch.equal(dws[0], dws[2])
    results = [_check(f"train {tag} forward", y, c["y_ref"][rows], FWD_BAR[dtype]),
               _check(f"train {tag} dx", dx, c["dx_ref"], FWD_BAR[dtype]),
               _check(f"train {tag} dW", dws[0], c["dw_ref"], WG_BAR[dtype])]
    assert all(ok for ok, _ in results), [msg for ok, msg in results if not ok]
    return lvl, L


@pytest.mark.parametrize("hint", HINTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("cin,cout", [(16, 32), (32, 64), (64, 128)])
def test_strided_layer_vs_oracle(dev, ran, cin, cout, dtype, hint):
    """3x3x3, stride 2, padding 1 on B = 2, (41, 24, 9): tiled forward, input gradient over the transposed table, staged-rows
    filter gradient over the metadata of the layer's table; output rows matched to the oracle's by coordinate."""
    c = _case(dev, cin, cout, dtype, "g41", False)
    _run_strided(dev, ran, c, cin, cout, dtype, hint, f"strided {cin}-{cout} {_name(dtype)} g41 hint {hint:g}")


@pytest.mark.parametrize("hint", [1.0, 8.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_stem_layer_vs_oracle(dev, ran, dtype, hint):
    """5 -> 16 SubM, rows zero-padded to 8 channels for the narrow forward kernel and to 16 for the staged-rows filter gradient
    (the extra rows of dW dropped); with and without the gradient of the voxel features."""
    c = _case(dev, 5, 16, dtype, "g40", True)
    tag = f"stem 5-16 {_name(dtype)} g40 hint {hint:g}"
    for needs_grad in (False, True):
        conv = _conv(dev, c, 5, 16, True)
        lvl, plan, L = _layer(dev, c, conv, dtype, hint, stem_needs_grad=needs_grad)
        assert L.variant == fused._SLAB_NARROW_SUBM and L.wg_code and L.wg_cin == 16
        x5 = c["x"].clone().requires_grad_(needs_grad)
        y = fused_train._LevelConv.apply(torch.nn.functional.pad(x5, (0, 3)), conv.weight, L)
        dx, dws = _three_backwards(y, c["gy"], conv, x5 if needs_grad else None)
        assert fused.geometry_status(lvl) == 0
        assert tuple(dws[0].shape) == (3, 3, 3, 5, 16) and torch.equal(dws[0], dws[1]) and torch.equal(dws[0], dws[2])
        results = [_check(f"train {tag} forward", y, c["y_ref"], FWD_BAR[dtype]),
                   _check(f"train {tag} dW", dws[0], c["dw_ref"], WG_BAR[dtype])]
        if needs_grad:
            assert tuple(dx.shape) == (c["n"], 5)
            results.append(_check(f"train {tag} dx", dx, c["dx_ref"], FWD_BAR[dtype]))
        else:
            assert lvl.index is None and not lvl.has("subm_neighbors")          # neither the hash index nor the int32 table was built
        assert all(ok for ok, _ in results), [msg for ok, msg in results if not ok]
    assert {r[3] for r in ran if r[0] == "slab"} == {fused._SLAB_NARROW_SUBM}
    _note(ran, hint)


def test_every_variant_the_training_path_selects_has_run(dev):
    """(last of the layer pins) The tables of spconv/fused.py decide what a training step launches between one and eight frames;
    every entry of them for the layers above must have produced a result that was compared."""
    slab = set().union(*[v for k, v in _RAN.items() if k[0] == "slab"] or [set()])
    tiled = {(k[1], k[2]): set() for k in _RAN if k[0] == "tiled"}
    for k, v in _RAN.items():
        if k[0] == "tiled":
            tiled[(k[1], k[2])] |= v
    for k in sorted(_RAN):
        print(f"{k[0]:5s} {k[1]:3d} -> {k[2]:3d} frames_hint {k[3]:g}: {sorted(_RAN[k])}")
    want = set(fused._SLAB_DEFAULT.values()) | set(fused._SLAB_DEFAULT_SMALL_BATCH.values()) | {fused._SLAB_NARROW_SUBM}
    hint = "(filled by the tests above: run the whole file, in order, in one process)"
    assert want <= slab, (sorted(want - slab), hint)
    pairs = [(16, 32), (32, 64), (64, 128), (32, 32), (64, 64), (128, 128)]
    for p in pairs:
        if p in fused._BATCHED_VARIANTS:
            assert fused._BATCHED_VARIANTS[p] in tiled.get(p, set()), (p, tiled.get(p), hint)
            assert 0 in tiled[p] or p[0] == p[1]               # ... and the default tiling below the cut (strided layers)
    assert [p for p in pairs if p in fused._BATCHED_VARIANTS], "the table lost the tested pairs"


# ---- the strided filter gradient next to the 16-bit slot limit -------------------------------------------------------------
def _dense(B, shape, keep=None):
    out = []
    for b in range(B):
        mask = np.ones(shape, bool) if keep is None else keep(b)
        lin = np.flatnonzero(mask.reshape(-1))
        out.append(np.concatenate([np.full((len(lin), 1), b), np.stack(np.unravel_index(lin, shape), 1)], 1))
    return np.concatenate(out).astype(np.int32)


def test_guarded_grid_keeps_the_gather_filter_gradient(dev, ran):
    """Dense B = 1, (3, 510, 130): 66 300 cells per x-plane, so the block that straddles the two output planes reads more than
    0xFFFE rows through kx = 1.  (Y = 512 would not do: its 256 * 65 outputs per plane are exactly 130 blocks, no block straddles,
    the longest range is 777 rows.)  The metadata kernel alone says so (status word); the layer does not take that metadata."""
    shape = (3, 510, 130)
    c = _case(dev, 16, 32, torch.float16, "dense guarded", False, (_dense(1, shape), 1, shape))
    assert c["n"] == 198900 and (c["m"] // 2) % 128 != 0
    # first: the case is what it claims — the metadata kernel alone, over the layer's table, reports the overflow
    conv = _conv(dev, c, 16, 32, False)
    lvl0, _, _ = _layer(dev, c, conv, torch.float16, 1.0, subm=False)
    out, nbr = lvl0.downsample((3, 3, 3), (2, 2, 2), (1, 1, 1), want_nbr=True)
    code = int(fused_train._capi.load().bevamd_spconv_wgrad_slab_block_rows(16))
    meta = ops.slab_build(nbr, out.n_cap, out.n_dev, code)
    assert int(meta.status.item()) != 0, "the case must overflow a range"
    _run_strided(dev, ran, c, 16, 32, torch.float16, 1.0, "strided 16-32 float16 dense (3,510,130) guarded", expect="gather")


def test_densest_admitted_grid_runs_the_staged_rows_filter_gradient(dev, ran):
    """Dense B = 1, (3, Y, 130) with the largest Y the guard admits: a range of about Y * 130 + 512 rows, just inside the slots."""
    Y = max(y for y in range(400, 512) if fused_train.strided_wgrad_route((3, y, 130), 1, 128) == "staged")
    assert fused_train.strided_wgrad_route((3, Y + 1, 130), 1, 128) == "gather" and Y * 130 > 0xFFFE - 4096
    shape = (3, Y, 130)
    c = _case(dev, 16, 32, torch.float16, "dense admitted", False, (_dense(1, shape), 1, shape))
    lvl, L = _run_strided(dev, ran, c, 16, 32, torch.float16, 1.0, f"strided 16-32 float16 dense (3,{Y},130) admitted")
    meta = lvl.down_slab_from_table((3, 3, 3), (2, 2, 2), (1, 1, 1), L.wg_code)
    nblk = (c["m"] + 127) // 128
    cnt = (meta.hdr[:nblk * 24].view(torch.int32).view(nblk, 3, 2)[:, :, 1] & 0x3FFFFFFF).cpu().numpy()
    assert cnt.max() > Y * 130, "the case must read a whole plane through one range"


def _seam(shape, filled):
    Y, Z = shape[1], shape[2]

    def keep(b):
        k = np.zeros(shape, bool)
        if b == 0:
            if filled:
                k[2] = k[3] = True
            else:
                k[2:4] = np.random.default_rng(8).random((2, Y, Z)) < 0.05
            k[1, 0, 0] = k[1, Y - 1, Z - 1] = True
        else:
            k[0, 0, 0] = k[1, 0, 0] = True
        return k
    return _dense(2, shape, keep)


def test_seam_overflow_is_caught_by_the_read_back_of_the_step(dev, ran):
    """B = 2, (4, 256, 130), an even X: the one place a range can exceed the one-plane bound is the block that holds the last rows
    of sample 0 and the first of sample 1 (kx = 0 spans the last two x-planes of sample 0).  Such grids take the staged-rows
    gradient with their status word in the step's read-back: filled planes set it and the step's filter gradient comes from the
    gather kernel, right; the same grid sparsely filled stays on the staged-rows kernel."""
    shape = (4, 256, 130)
    assert fused_train.strided_wgrad_route(shape, 2, 128) == "checked"
    c = _case(dev, 16, 32, torch.float16, "seam filled", False, (_seam(shape, True), 2, shape))
    lvl, L = _run_strided(dev, ran, c, 16, 32, torch.float16, 1.0, "strided 16-32 float16 seam (4,256,130) filled", expect="caught")
    assert fused.geometry_status(lvl) == 0                      # the word was cleared for the next pass
    del ran[:]
    c = _case(dev, 16, 32, torch.float16, "seam sparse", False, (_seam(shape, False), 2, shape))
    lvl, L = _run_strided(dev, ran, c, 16, 32, torch.float16, 1.0, "strided 16-32 float16 seam (4,256,130) sparse")
    assert L.wg_checked and L.wg_code
