"""The float64 BatchNorm reference of tests/bn_reference.py, checked on the host (no GPU):
  * its closed forms against torch.nn.BatchNorm1d (+ add, + ReLU) in float64 through autograd: 1e-12 relative;
  * a plain numpy float32 evaluation of the same formulas, rounded where the kernels round, stays inside the elementwise bounds that
    tests/test_gpu_sparse_bn_float64.py enforces, and differs from the mirror in at most 1e-3 of the 16-bit elements, on reduced-row
    versions of every 16-bit input set of that module: an fp32 implementation meets both conditions at these sizes (over
    millions of 16-bit elements with a residual it meets a two-ulp tie flip of t1 + res about once per million, which is why the
    kernel evaluates t1 in fp64 there: that module's docstring);
  * the launch-grid facts of the edge cases, from the constants read in csrc/sparse_bn.hip."""
import numpy as np
import pytest
import torch
from torch import nn

import bn_reference as R

CPU = torch.device("cpu")
SHARE_CAP = 1e-3


def _close(a, b, what):
    a, b = a.detach().double(), b.detach().double()
    err = float((a - b).abs().max())
    assert err <= 1e-12 * (1.0 + float(b.abs().max())), (what, err)


CLOSED_FORM_CASES = {
    "relu_res": dict(n=300, relu=True, res=True),
    "relu": dict(n=300, relu=True, res=False),
    "res": dict(n=300, relu=False, res=True),
    "plain": dict(n=300, relu=False, res=False),
    "constant_channel": dict(n=300, relu=True, res=True, constant=True),
    "two_rows": dict(n=2, relu=True, res=True),
    "negative_and_zero_weight": dict(n=300, relu=True, res=True, weight="signed"),
}


@pytest.mark.parametrize("case", sorted(CLOSED_FORM_CASES))
def test_closed_forms_against_torch_float64(case):
    k = CLOSED_FORM_CASES[case]
    n, c, eps, momentum = k["n"], 8, 1e-3, 0.01
    g = torch.Generator().manual_seed(7)
    x = torch.randn((n, c), generator=g, dtype=torch.float64) * 1.7 + 0.3
    if k.get("constant"):
        x[:, 2] = 3.25
    res = torch.randn((n, c), generator=g, dtype=torch.float64) if k["res"] else None
    dy = torch.randn((n, c), generator=g, dtype=torch.float64)
    w = torch.linspace(0.5, 1.5, c, dtype=torch.float64)
    if k.get("weight") == "signed":
        w = torch.tensor([-2.0, -0.5, 0.0, 0.25, 1.0, -1.5, 3.0, 0.0], dtype=torch.float64)
    b = torch.linspace(-0.2, 0.2, c, dtype=torch.float64)

    m = nn.BatchNorm1d(c, eps=eps, momentum=momentum).double().train()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
        m.running_mean.fill_(0.1)
        m.running_var.fill_(0.9)
    rm0, rv0 = m.running_mean.clone(), m.running_var.clone()
    xt = x.clone().requires_grad_(True)
    rt = res.clone().requires_grad_(True) if res is not None else None
    yt = m(xt)
    if rt is not None:
        yt = yt + rt
    if k["relu"]:
        yt = torch.relu(yt)
    yt.backward(dy)

    M = R.moments64(x, eps, momentum, rm0, rv0)
    F = R.forward_mirror(x, M["mean"], M["invstd"], w, b, res, k["relu"], torch.float32)
    mask = ~(F["y"] <= 0) if k["relu"] else None
    B = R.backward_mirror(x, dy, mask, M["mean"], M["invstd"], w, torch.float32)
    _close(F["y"], yt, "y")
    _close(B["dx"], xt.grad, "dx")
    _close(B["dweight"], m.weight.grad, "dweight")
    _close(B["dbias"], m.bias.grad, "dbias")
    if rt is not None:
        _close(B["dz"], rt.grad, "dres")
    _close(M["running_mean"], m.running_mean, "running_mean")
    _close(M["running_var"], m.running_var, "running_var")
    if k.get("constant"):
        assert float(M["var"][2]) == 0.0 and float(M["invstd"][2]) == 1.0 / np.sqrt(eps)
        assert torch.equal(F["t1"][:, 2], b[2].expand(n))


def test_rounding_to_the_storage_types_is_one_rounding():
    g = torch.Generator().manual_seed(0)
    a32 = torch.cat([torch.randn(20000, generator=g) * s for s in (1e-7, 1e-3, 1.0, 300.0, 7e4)])
    a = a32.double()                       # fp32 values: fp32 -> 16 bit is then a single rounding in torch as well
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(R.round_dt(a, dt), a32.to(dt).double())
        r = a32.to(dt)
        nxt = (r.abs().view(torch.int16) + 1).view(dt).double()                # the next value of the storage type, by its bits
        ok = torch.isfinite(r) & torch.isfinite(nxt)
        assert torch.equal(R.ulp(r.double(), dt)[ok], (nxt - r.abs().double())[ok])
    # a tie of the float64 value that fp32 in between would break the wrong way: 1 + 2^-11 + 2^-30 lies above the fp16 tie
    v = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30], dtype=torch.float64)
    assert float(R.round_dt(v, torch.float16)) == 1.0 + 2.0 ** -10
    assert float(v.float().half()) == 1.0                                      # the double rounding the helper avoids
    assert torch.equal(R.round_dt(v, torch.float32), v)
    assert float(R.ulp(torch.tensor([0.0], dtype=torch.float64), torch.float16)) == 2.0 ** -24


def _np(t):
    return t.detach().float().numpy()


def fp32_pipeline(inp, dtype, relu, eps=1e-3):
    """The kernels' arithmetic in plain numpy float32 (no fused multiply-add, numpy's own summation order), rounded to the storage
    type where the kernels round."""
    def rnd(a):
        return torch.from_numpy(a).to(dtype).float().numpy() if dtype != torch.float32 else a

    x, dy = _np(inp["x"]), _np(inp["dy"])
    w, b = _np(inp["weight"]), _np(inp["bias"])
    n = x.shape[0]
    M = R.moments64(inp["x"], eps)
    mean, invstd = M["mean"].float().numpy(), M["invstd"].float().numpy()
    sc = invstd * w
    t1 = rnd((x - mean) * sc + b)
    t2 = rnd(t1 + _np(inp["res"])) if inp["res"] is not None else t1
    y = np.where(t2 <= 0, np.float32(0), t2) if relu else t2
    dz = np.where(y <= 0, np.float32(0), dy) if relu else dy
    xhat = (x - mean) * invstd
    s1, s2 = dz.sum(0, dtype=np.float32), (dz * xhat).sum(0, dtype=np.float32)
    inv_n = np.float32(1.0) / np.float32(n)
    dx = rnd((w * invstd) * (dz - s1 * inv_n - xhat * (s2 * inv_n)))
    T = torch.from_numpy
    return dict(y=T(y), t1=T(t1), dx=T(dx), dres=T(dz), mean=T(mean), invstd=T(invstd), sum_dz=T(s1), sum_dz_xhat=T(s2))


def check_against_mirror(inp, out, dtype, relu):
    """The elementwise conditions of the GPU module on one result set; returns the shares of y and dx that differ from the mirror."""
    F = R.forward_mirror(inp["x"], out["mean"], out["invstd"], inp["weight"], inp["bias"], inp["res"], relu, dtype)
    y = out["y"].double()
    assert bool(((y - F["y"]).abs() <= F["bound"]).all()), float(((y - F["y"]).abs() - F["bound"]).max())
    mask = ~(y <= 0) if relu else None
    B = R.backward_mirror(inp["x"], inp["dy"], mask, out["mean"], out["invstd"], inp["weight"], dtype, out["sum_dz"], out["sum_dz_xhat"])
    dx = out["dx"].double()
    assert bool(((dx - B["dx"]).abs() <= B["dx_bound"]).all()), float(((dx - B["dx"]).abs() - B["dx_bound"]).max())
    assert torch.equal(out["dres"].double(), B["dz"])
    return float((y != F["y"]).double().mean()), float((dx != B["dx"]).double().mean())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n,c", [(1000, 8), (257, 256), (2, 256), (7, 8)])
@pytest.mark.parametrize("relu,with_res", [(True, True), (False, True), (True, False)])
def test_fp32_evaluation_meets_the_elementwise_bounds_and_the_share_cap(dtype, n, c, relu, with_res):
    inp = R.standard_inputs(CPU, n, c, dtype, with_res=with_res)
    out = fp32_pipeline(inp, dtype, relu)
    share_y, share_dx = check_against_mirror(inp, out, dtype, relu)
    if dtype != torch.float32 and n * c >= 8000:
        assert share_y <= SHARE_CAP, share_y


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_fp32_evaluation_of_the_planted_relu_boundary(dtype):
    inp = R.standard_inputs(CPU, 1000, 64, dtype)
    t1 = fp32_pipeline(dict(inp, res=None), dtype, relu=False)["y"].to(dtype)
    planted, idx = R.plant_relu_boundary(inp, t1)
    out = fp32_pipeline(planted, dtype, relu=True)
    assert idx.numel() == 200 and idx.unique().numel() == 200
    assert bool((out["y"].reshape(-1)[idx] == 0).all()) and bool((out["dres"].reshape(-1)[idx] == 0).all())
    assert bool((planted["dy"].reshape(-1)[idx] != 0).all())           # a mask `y < 0` would let these through
    share_y, _ = check_against_mirror(planted, out, dtype, relu=True)
    if dtype != torch.float32:
        assert share_y <= SHARE_CAP, share_y


# (dtype, c, n): slabs, ticket groups, empty trailing slabs, second grid-stride trip — the edges tests/test_gpu_sparse_bn_float64.py runs
GRID_EDGES = [
    (torch.float32, 4, 2, (1, 1, 0, False)), (torch.float32, 4, 4097, (1, 1, 0, False)), (torch.float32, 4, 8193, (2, 1, 0, False)),
    (torch.float32, 256, 2, (1, 1, 0, False)), (torch.float32, 256, 3, (1, 1, 0, False)), (torch.float32, 256, 65, (1, 1, 0, False)),
    (torch.float32, 256, 129, (2, 1, 0, False)), (torch.float32, 256, 2048, (32, 1, 0, False)),
    (torch.float32, 256, 2112, (33, 2, 0, False)), (torch.float32, 256, 16384, (256, 8, 0, False)),
    (torch.float32, 256, 16385, (256, 8, 3, False)), (torch.float32, 256, 70001, (256, 8, 0, True)),
    (torch.float16, 8, 2, (1, 1, 0, False)), (torch.float16, 8, 4100, (1, 1, 0, False)), (torch.float16, 256, 7, (1, 1, 0, False)),
    (torch.float16, 256, 4224, (33, 2, 0, False)), (torch.float16, 256, 32769, (256, 8, 1, False)),
    (torch.float16, 256, 131075, (256, 8, 0, True)),
]


def test_grid_facts_of_the_edge_cases():
    k = R.source_constants()
    assert k == dict(threads=256, group=32, max_slabs=1024, default_slabs=256, rows_per_lane=16, apply_cap=4096)
    for dtype, c, n, want in GRID_EDGES:
        f = R.grid_facts(n, c, dtype, k=k)
        assert (f["slabs"], f["groups"], f["empty"], f["second_trip"]) == want, (dtype, c, n, f)
    # a retune moves them: another slab cap, group size or grid cap changes the facts of the cases that sit on that edge
    assert R.grid_facts(16385, 256, torch.float32, k=dict(k, default_slabs=192))["empty"] != 3
    assert R.grid_facts(2112, 256, torch.float32, k=dict(k, group=64))["groups"] == 1
    assert not R.grid_facts(70001, 256, torch.float32, k=dict(k, apply_cap=8192))["second_trip"]
    f = R.grid_facts(65537, 256, torch.float32, slabs=1024, k=k)
    assert (f["slabs"], f["groups"], f["empty"]) == (1024, 32, 15)
