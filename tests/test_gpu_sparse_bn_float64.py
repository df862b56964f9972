"""GPU: the sparse BatchNorm kernels (csrc/sparse_bn.hip) against the float64 reference of tests/bn_reference.py, at the edges of their
launch grids and of their values.  Everything goes through `bn._BnAct.apply` / `bn_act`.

Statistics and parameter gradients are judged per channel against float64, each on its natural scale:
    mean, running_mean   |err| / sqrt(var64 + eps)          invstd, running_var   relative
    d weight             |err| / sum |dz * xhat|            d bias                |err| / sum |dz|
(the largest over channels).  The bar is measured, not chosen: on the same GPU and inputs `nn.BatchNorm1d` + add + relu run (under
autocast for 16-bit rows) and the kernel's error must not exceed 4 x torch's, with a floor of 2e-6 (tests/test_gpu_decoder_layer.py).
The two sum in different orders, and at rounding-noise level the ratio of two independent errors wanders by a few times; a kernel
that loses a digit still fails.  Both errors go through conftest.record_parity: `<case>` the kernel's, `<case>_torch` torch's.
The sums behind d weight / d bias are taken with each implementation's own stored mean, invstd and ReLU mask: the reduction is
judged apart from the statistics.

Elementwise outputs are judged against the mirror fed with the kernel's own mean, invstd, d weight, d bias and mask:
    d residual   bit-equal to dy * (y > 0)  (dy itself without ReLU)
    y            within one storage ulp of max(|t1|, |t2|) + 2^-20 * (|x - mean| * |invstd * w| + |b| + |res|)
    dx           within one storage ulp of the reference + 2^-20 * |w * invstd| * (|dz| + |mean dz| + |xhat * mean(dz * xhat)|)
    16-bit y     at most 1e-3 of the elements differ from the mirror at all (tests/test_bn_reference.py: a correct fp32
                 implementation differs in ~2e-5 of fp16 and ~1e-6 of bf16 elements)

The bound on y and round-half-even.  Where the float64 value of t1 lies within fp32 rounding of a tie of the storage type, an fp32
pipeline rounds t1 to the other neighbour (one ulp, allowed; 7e-5 of the fp16 elements).  Where t1 + res is then itself an exact tie
— the residual has finer bits than t1 — the two sums are ties one ulp apart, and round-half-even sends them to even neighbours TWO
ulps apart, e.g. x = 1.8349609375, res = -0.309814453125: t1 = 0.85546875 | 0.85498046875, t1 + res = 1117.5 | 1116.5 ulps,
y = 1118 | 1116 ulps.  With t1 evaluated in fp32 the kernel missed the bound at 8 of 8 388 864 (n = 32769) and 19 of 33 555 200
(n = 131075) fp16 elements, `nn.BatchNorm1d` + add + relu under autocast at 7 and 35.  For 16-bit rows with a residual the kernel
therefore evaluates t1 in fp64 and rounds it once (csrc/sparse_bn.hip, bn_apply_kernel<DT, true>); the bound holds everywhere.

Run as a program (`python test_gpu_sparse_bn_float64.py --knobs`, started by test_knob_paths_in_a_child_process with
BEVAMD_BN_UNROLL=8 and BEVAMD_BN_SLABS=1024 in its environment) it runs the knob shapes and prints one JSON line of errors and bars.
"""
import json
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)          # the child process starts in tests/

import bn_reference as R  # noqa: E402
from bevfusion_amd.spconv import bn as native_bn  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR, FACTOR, SHARE_CAP = 2e-6, 4.0, 1e-3
NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}


def _ratio(err, scale):
    """max over channels of err / scale;  0 / 0 = 0 (a constant channel's d weight), x / 0 = inf."""
    q = torch.where(scale > 0, err / scale, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(q.max())


def _module(dev, inp, eps, momentum):
    c = inp["x"].shape[1]
    m = nn.BatchNorm1d(c, eps=eps, momentum=momentum).to(dev).train()
    with torch.no_grad():
        m.weight.copy_(inp["weight"])
        m.bias.copy_(inp["bias"])
        m.running_mean.fill_(0.1)
        m.running_var.fill_(0.9)
    return m


def run_native(dev, inp, relu, eps=1e-3, momentum=0.01):
    """One forward + backward on the kernels: every output, gradient and updated buffer."""
    m = _module(dev, inp, eps, momentum)
    x = inp["x"].clone().requires_grad_(True)
    res = inp["res"].clone().requires_grad_(True) if inp["res"] is not None else None
    assert native_bn.usable(m, x, res)
    y, mean, invstd = native_bn._BnAct.apply(x, m.weight, m.bias, res, m.running_mean, m.running_var, eps, momentum, relu)
    y.backward(inp["dy"])
    return dict(y=y.detach(), mean=mean, invstd=invstd, dx=x.grad, dres=res.grad if res is not None else None, dweight=m.weight.grad,
                dbias=m.bias.grad, running_mean=m.running_mean.detach(), running_var=m.running_var.detach())


def run_torch(dev, inp, relu, eps=1e-3, momentum=0.01):
    """The same on torch's modules.  The batch mean / variance torch normalises with are read off a second module with momentum 1
    (its running statistics then ARE the batch statistics)."""
    dtype = inp["x"].dtype
    n = inp["x"].shape[0]
    m, probe = _module(dev, inp, eps, momentum), _module(dev, inp, eps, 1.0)
    x = inp["x"].clone().requires_grad_(True)
    res = inp["res"].clone().requires_grad_(True) if inp["res"] is not None else None
    with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
        y = m(x)
        if res is not None:
            y = y + res
        if relu:
            y = torch.relu(y)
        with torch.no_grad():
            probe(inp["x"])
    assert y.dtype == dtype
    y.backward(inp["dy"])
    var = probe.running_var.double() * ((n - 1.0) / n)
    return dict(y=y.detach(), mean=probe.running_mean.detach(), invstd=1.0 / torch.sqrt(var + eps), dweight=m.weight.grad, dbias=m.bias.grad,
                running_mean=m.running_mean.detach(), running_var=m.running_var.detach())


def statistic_errors(inp, out, relu, eps=1e-3, momentum=0.01):
    """The six per-channel error figures of one implementation's results against float64."""
    M = R.moments64(inp["x"], eps, momentum, torch.full_like(out["mean"], 0.1), torch.full_like(out["mean"], 0.9))
    sd = torch.sqrt(M["var"] + eps)
    mask = ~(out["y"] <= 0) if relu else None
    B = R.backward_mirror(inp["x"], inp["dy"], mask, out["mean"], out["invstd"], inp["weight"], inp["x"].dtype)
    one = torch.ones_like(sd)
    return dict(mean=_ratio((out["mean"].double() - M["mean"]).abs(), sd),
                invstd=_ratio((out["invstd"].double() - M["invstd"]).abs(), M["invstd"]),
                running_mean=_ratio((out["running_mean"].double() - M["running_mean"]).abs(), sd),
                running_var=_ratio((out["running_var"].double() - M["running_var"]).abs(), M["running_var"].abs() * one),
                dweight=_ratio((out["dweight"].double() - B["dweight"]).abs(), B["abs_dzx"]),
                dbias=_ratio((out["dbias"].double() - B["dbias"]).abs(), B["abs_dz"]))


def elementwise_problems(inp, out, relu, theirs=None):
    """The elementwise conditions on the kernel's y, dx and d residual; a list of what is violated."""
    dtype = inp["x"].dtype
    bad = []
    F = R.forward_mirror(inp["x"], out["mean"], out["invstd"], inp["weight"], inp["bias"], inp["res"], relu, dtype)
    y = out["y"].double()
    over = (y - F["y"]).abs() - F["bound"]
    if not bool((over <= 0).all()):          # a NaN on either side fails as well
        bad.append(f"y outside its bound at {int((~(over <= 0)).sum())} of {y.numel()} elements (worst excess {float(over.nan_to_num(nan=float('inf')).max()):.3e})")
        if theirs is not None:               # for the reader of a failure: torch's own y against the same bound, from torch's own statistics
            Ft = R.forward_mirror(inp["x"], theirs["mean"], theirs["invstd"].float(), inp["weight"], inp["bias"], inp["res"], relu, dtype)
            bad[-1] += f"; torch's y: {int((~((theirs['y'].double() - Ft['y']).abs() <= Ft['bound'])).sum())} elements"
    if dtype != torch.float32:
        share = float((y != F["y"]).double().mean())
        if share > SHARE_CAP:
            bad.append(f"{share:.3e} of the 16-bit elements of y differ from the mirror (cap {SHARE_CAP})")
    mask = ~(out["y"] <= 0) if relu else None
    B = R.backward_mirror(inp["x"], inp["dy"], mask, out["mean"], out["invstd"], inp["weight"], dtype, out["dbias"], out["dweight"])
    over = (out["dx"].double() - B["dx"]).abs() - B["dx_bound"]
    if not bool((over <= 0).all()):
        bad.append(f"dx outside its bound at {int((~(over <= 0)).sum())} of {y.numel()} elements (worst excess {float(over.nan_to_num(nan=float('inf')).max()):.3e})")
    if out["dres"] is not None:
        want = torch.where(out["y"] > 0, inp["dy"], torch.zeros_like(inp["dy"])) if relu else inp["dy"]
        ints = torch.int32 if dtype == torch.float32 else torch.int16
        if not torch.equal(out["dres"].view(ints), want.view(ints)):
            bad.append("d residual is not dy * (y > 0) bit for bit")
    return bad


def judge(dev, inp, relu, eps=1e-3, momentum=0.01):
    """Run both implementations on one input set.  Returns ({quantity: (kernel error, torch error, bar)}, [violations], outputs)."""
    ours, theirs = run_native(dev, inp, relu, eps, momentum), run_torch(dev, inp, relu, eps, momentum)
    e_ours, e_torch = statistic_errors(inp, ours, relu, eps, momentum), statistic_errors(inp, theirs, relu, eps, momentum)
    figures = {q: (e_ours[q], e_torch[q], max(FACTOR * e_torch[q], FLOOR)) for q in e_ours}
    bad = [f"{q}: error {e:.3e} against float64, torch {t:.3e}, bar {bar:.3e}" for q, (e, t, bar) in figures.items() if not e <= bar]
    return figures, bad + elementwise_problems(inp, ours, relu, theirs), ours


def check(dev, case, inp, relu, eps=1e-3, momentum=0.01, after=None):
    from conftest import record_parity

    figures, bad, ours = judge(dev, inp, relu, eps, momentum)
    for q, (e, t, bar) in figures.items():
        print(f"sparse_bn/{case}/{q}: kernel {e:.3e} torch {t:.3e} bar {bar:.3e}")
        record_parity(f"sparse_bn/{case}/{q}", e, bar)
        record_parity(f"sparse_bn/{case}/{q}_torch", t, bar)
    if after is not None:
        after(ours)                    # the case's own assertions, before the common ones can fail
    assert not bad, (case, bad)
    return ours


def test_reference_rounds_on_the_device_as_on_the_host(dev):
    """tests/test_bn_reference.py checks the float64 helpers on the host; the cases here evaluate them on the device."""
    g = torch.Generator().manual_seed(0)
    a = torch.cat([torch.randn(20000, generator=g, dtype=torch.float64) * s for s in (1e-7, 1e-3, 1.0, 300.0, 7e4)] + [torch.zeros(1, dtype=torch.float64)])
    for dt in NAME:
        assert torch.equal(R.round_dt(a.to(dev), dt).cpu(), R.round_dt(a, dt)) and torch.equal(R.ulp(a.to(dev), dt).cpu(), R.ulp(a, dt))
    x = torch.randn((3001, 8), generator=g, dtype=torch.float64) * 3.0 + 100.0
    M, Md = R.moments64(x, 1e-3), R.moments64(x.to(dev), 1e-3)
    assert all(float(((Md[k].cpu() - M[k]).abs() / M[k].abs()).max()) <= 1e-13 for k in M)


# ---- grid edges: (c, n, slabs, ticket groups, empty trailing slabs, second grid-stride trip of the elementwise kernels) ----
FP32_EDGES = [
    (4, 2, 1, 1, 0, False), (4, 4097, 1, 1, 0, False), (4, 8193, 2, 1, 0, False),             # one lane per row; ragged trip; G = 2
    (256, 2, 1, 1, 0, False), (256, 3, 1, 1, 0, False),                                       # fewer rows than rows in flight
    (256, 65, 1, 1, 0, False), (256, 129, 2, 1, 0, False),
    (256, 2048, 32, 1, 0, False),                                                             # one full ticket group
    (256, 2112, 33, 2, 0, False),                                                             # a second group of one slab
    (256, 16384, 256, 8, 0, False),                                                           # the slab cap
    (256, 16385, 256, 8, 3, False),                                                           # the cap with 65 rows per slab: slabs 253 .. 255 own no rows
    (256, 70001, 256, 8, 0, True),
]
HALF_EDGES = [
    (8, 2, 1, 1, 0, False), (8, 4100, 1, 1, 0, False), (256, 7, 1, 1, 0, False), (256, 4224, 33, 2, 0, False),
    (256, 32769, 256, 8, 1, False),                                                           # the cap, last slab empty
]
FP16_ONLY = [(256, 131075, 256, 8, 0, True)]
EDGES = ([(torch.float32,) + e for e in FP32_EDGES] + [(torch.float16,) + e for e in HALF_EDGES + FP16_ONLY] +
         [(torch.bfloat16,) + e for e in HALF_EDGES])


def _assert_grid(dtype, c, n, slabs, groups, empty, second_trip, cap=None):
    f = R.grid_facts(n, c, dtype, slabs=cap)
    assert (f["slabs"], f["groups"], f["empty"], f["second_trip"]) == (slabs, groups, empty, second_trip), (NAME[dtype], c, n, f)


@pytest.mark.parametrize("dtype,c,n,slabs,groups,empty,second_trip", EDGES, ids=[f"{NAME[e[0]]}-{e[1]}-{e[2]}" for e in EDGES])
def test_grid_edges(dev, dtype, c, n, slabs, groups, empty, second_trip):
    _assert_grid(dtype, c, n, slabs, groups, empty, second_trip)
    check(dev, f"edge/{NAME[dtype]}/c{c}/n{n}", R.standard_inputs(dev, n, c, dtype), relu=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("relu,with_res", [(False, True), (True, False), (False, False)], ids=["no_relu", "no_residual", "plain"])
def test_without_relu_or_residual(dev, dtype, relu, with_res):
    n, c = (2112, 256) if dtype == torch.float32 else (4224, 256)
    check(dev, f"edge/{NAME[dtype]}/c{c}/n{n}/relu{int(relu)}_res{int(with_res)}", R.standard_inputs(dev, n, c, dtype, with_res=with_res), relu)


# ---- value edges, at (fp32, 64, 5000) unless noted ----
def _fp32_set(dev, x, weight=None, seed=0):
    n, c = x.shape
    g = torch.Generator(device=dev).manual_seed(77 + seed)
    return dict(x=x, res=torch.randn((n, c), generator=g, device=dev), dy=torch.randn((n, c), generator=g, device=dev),
                weight=weight if weight is not None else torch.linspace(0.5, 1.5, c, device=dev), bias=torch.linspace(-0.2, 0.2, c, device=dev))


def _randn(dev, n, c, seed):
    return torch.randn((n, c), generator=torch.Generator(device=dev).manual_seed(seed), device=dev)


def test_channel_scales_over_six_decades(dev):
    """Channel std logspace(-3, 3), means up to 100 std, weights +-logspace(-2, 2) with one exact zero: a channel 1e6 below the largest
    is judged on its own scale."""
    n, c = 5000, 64
    std = torch.logspace(-3, 3, c, device=dev)
    mean = std * torch.linspace(-100.0, 100.0, c, device=dev).roll(17)
    w = torch.logspace(-2, 2, c, device=dev) * torch.where(torch.arange(c, device=dev) % 2 == 0, 1.0, -1.0)
    w[5] = 0.0
    inp = _fp32_set(dev, _randn(dev, n, c, 5) * std + mean, weight=w)
    inp["res"] = inp["res"] * w.abs()            # a residual of the channel's own output scale
    check(dev, "value/channel_scales", inp, relu=True)


def test_constant_channel(dev):
    n, c, eps = 5000, 64, 1e-3
    x = _randn(dev, n, c, 6) * 1.7 + 0.3
    x[:, 9] = 3.25
    inp = _fp32_set(dev, x)
    inp["res"] = None
    ours = check(dev, "value/constant_channel", inp, relu=False)
    eps32 = float(torch.tensor(eps, dtype=torch.float32))                                          # the launcher takes eps as a float
    assert float(ours["mean"][9]) == 3.25 and float(ours["invstd"][9]) == float(torch.tensor(1.0 / eps32 ** 0.5, dtype=torch.float32))
    assert torch.equal(ours["y"][:, 9], inp["bias"][9].expand(n))                                 # y = bias
    dz = inp["dy"][:, 9].double()
    want = float(inp["weight"][9]) * float(ours["invstd"][9]) * (dz - dz.mean())                   # dx = w * invstd * (dz - mean dz)
    assert float((ours["dx"][:, 9].double() - want).abs().max()) <= 2.0 ** -20 * float(want.abs().max())
    assert float(ours["dweight"][9]) == 0.0


def test_large_mean_forward_and_backward(dev):
    """|mean| up to 300 at std 0.05 .. 2 (tests/test_gpu_sparse_bn.py checks the running variance only)."""
    n, c = 5000, 64
    x = _randn(dev, n, c, 8) * torch.linspace(0.05, 2.0, c, device=dev) + torch.linspace(-300.0, 300.0, c, device=dev)
    check(dev, "value/large_mean", _fp32_set(dev, x), relu=True, eps=1e-5, momentum=0.1)


@pytest.mark.parametrize("n", [5000, 50000])
@pytest.mark.parametrize("where", ["row0", "middle"])
def test_one_outlying_row_wherever_it_sits(dev, n, where):
    """N(0, 1) with ONE row of +50 in every channel, at row 0 or at row n / 2: the statistics meet the same bars at both places.  (Sums
    shifted by row 0 alone lose ~5e-5 of the variance when that row lies 50 sigma out: q = sum (x - 50)^2 is 2500 n, of which the
    variance is the 1 / 2500 that survives the subtraction of (p / n)^2.)"""
    c = 64
    x = _randn(dev, n, c, 9)
    x[0 if where == "row0" else n // 2] = 50.0
    check(dev, f"value/outlier_{where}/n{n}", _fp32_set(dev, x), relu=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_relu_boundary(dev, dtype):
    """Residual = -t1 at 200 places (exact in the storage type): y is exactly zero there, and zero is masked (torch: y <= 0)."""
    n, c = 5000, 64
    inp = R.standard_inputs(dev, n, c, dtype)
    t1 = run_native(dev, dict(inp, res=None), relu=False)["y"]
    planted, idx = R.plant_relu_boundary(inp, t1)
    assert idx.numel() == 200 and bool((planted["dy"].reshape(-1)[idx] != 0).all())

    def at_the_planted_places(ours):
        assert bool((ours["y"].reshape(-1)[idx] == 0).all())
        assert bool((ours["dres"].reshape(-1)[idx] == 0).all())
        # dx there is the mirror's with dz = 0: `check` uses the mask of the kernel's own y, which is False at these places
        assert not bool((~(ours["y"] <= 0)).reshape(-1)[idx].any())

    check(dev, f"value/relu_boundary/{NAME[dtype]}", planted, relu=True, after=at_the_planted_places)


@pytest.mark.parametrize("row", [0, 1234, 2500, 4999])          # the rows the statistics take their pivot from, and another
def test_nan_stays_in_its_channel(dev, row):
    n, c = 5000, 64
    inp = _fp32_set(dev, _randn(dev, n, c, 10) * 1.7 + 0.3)
    clean = run_native(dev, inp, relu=True)
    x = inp["x"].clone()
    x[row, 3] = float("nan")
    dirty = run_native(dev, dict(inp, x=x), relu=True)
    others = [ch for ch in range(c) if ch != 3]
    for k in clean:
        a, b = clean[k][..., others], dirty[k][..., others]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    # what torch gives as well: NaN statistics, outputs and input / weight gradients in the channel; d bias = sum of the unmasked dy
    for k in ("y", "dx", "mean", "invstd", "running_mean", "running_var", "dweight"):
        assert bool(torch.isnan(dirty[k][..., 3]).all()), k
    theirs = run_torch(dev, dict(inp, x=x), relu=True)
    for k in ("y", "mean", "invstd", "running_mean", "running_var", "dweight"):
        assert bool(torch.isnan(theirs[k][..., 3]).all()), k


def test_three_training_steps_on_one_module(dev):
    """n = 2112, 65, 16385 at C = 256 fp32: 33, 1 and 256 slabs on one cached workspace.  After each step the running statistics follow
    the float64 recurrence (bars from a torch module stepping beside it) and num_batches_tracked counts."""
    from conftest import record_parity

    c, eps, momentum = 256, 1e-3, 0.01
    for n, slabs in ((2112, 33), (65, 1), (16385, 256)):
        assert R.grid_facts(n, c, torch.float32)["slabs"] == slabs
    ours = nn.BatchNorm1d(c, eps=eps, momentum=momentum).to(dev).train()
    theirs = nn.BatchNorm1d(c, eps=eps, momentum=momentum).to(dev).train()
    rm, rv = torch.zeros(c, dtype=torch.float64, device=dev), torch.ones(c, dtype=torch.float64, device=dev)
    for step, n in enumerate((2112, 65, 16385)):
        inp = R.standard_inputs(dev, n, c, torch.float32, seed=step)
        y = native_bn.bn_act(inp["x"], ours, relu=True, residual=inp["res"])
        yt = torch.relu(theirs(inp["x"]) + inp["res"])
        M = R.moments64(inp["x"], eps, momentum, rm, rv)
        rm, rv = M["running_mean"], M["running_var"]
        sd = torch.sqrt(M["var"] + eps)
        for q, want, scale in (("running_mean", rm, sd), ("running_var", rv, rv)):
            e, t = (_ratio((getattr(m, q).double() - want).abs(), scale) for m in (ours, theirs))
            bar = max(FACTOR * t, FLOOR)
            print(f"sparse_bn/three_steps/step{step}/{q}: kernel {e:.3e} torch {t:.3e} bar {bar:.3e}")
            record_parity(f"sparse_bn/three_steps/step{step}/{q}", e, bar)
            record_parity(f"sparse_bn/three_steps/step{step}/{q}_torch", t, bar)
            assert e <= bar, (step, q, e, t)
        assert float((y - yt).detach().abs().max()) <= 2e-5 * (1.0 + float(yt.detach().abs().max()))
    assert int(ours.num_batches_tracked) == int(theirs.num_batches_tracked) == 3


# ---- the knob paths: BEVAMD_BN_UNROLL=8 and BEVAMD_BN_SLABS=1024 are read once per process ----
KNOBS = dict(BEVAMD_BN_UNROLL="8", BEVAMD_BN_SLABS="1024")
KNOB_CASES = [                                                                   # under BEVAMD_BN_SLABS=1024
    (torch.float32, 256, 65537, 1024, 32, 15, True),                             # MAX_SLABS in MAX_GROUPS groups, 15 empty trailing slabs
    (torch.float16, 256, 65537, 512, 16, 3, False),
    (torch.float16, 256, 131073, 1024, 32, 7, True),                             # the same edge at 8 channels per lane
    (torch.float32, 256, 2112, 33, 2, 0, False), (torch.float16, 256, 2112, 16, 1, 0, False),
    (torch.float32, 4, 4097, 1, 1, 0, False), (torch.float16, 8, 4097, 1, 1, 0, False),
]


def knob_child():
    assert all(os.environ.get(k) == v for k, v in KNOBS.items()), "the knobs must be in the environment before the library loads"
    dev = torch.device("cuda:0")
    report, failed = {}, []
    for dtype, c, n, *facts in KNOB_CASES:
        _assert_grid(dtype, c, n, *facts, cap=int(KNOBS["BEVAMD_BN_SLABS"]))
        figures, bad, _ = judge(dev, R.standard_inputs(dev, n, c, dtype), relu=True)
        case = f"knobs/{NAME[dtype]}/c{c}/n{n}"
        report[case] = figures
        failed += [(case, b) for b in bad]
    print("BN-KNOBS " + json.dumps(report))
    print("BN-KNOBS-OK" if not failed else f"BN-KNOBS-FAILED {failed}")
    return 0 if not failed else 1


def test_knob_paths_in_a_child_process(dev):
    """The unroll-8 instantiations and 1024 slabs (32 ticket groups) in a fresh process that has the knobs in its environment."""
    from conftest import record_parity

    assert R.source_constants()["max_slabs"] == int(KNOBS["BEVAMD_BN_SLABS"])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--knobs"], capture_output=True, text=True, timeout=170,
                       env=dict(os.environ, **KNOBS))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("BN-KNOBS ")]
    for case, figures in (json.loads(lines[-1][len("BN-KNOBS "):]) if lines else {}).items():
        for q, (e, t, bar) in figures.items():
            print(f"sparse_bn/{case}/{q}: kernel {e:.3e} torch {t:.3e} bar {bar:.3e}")
            record_parity(f"sparse_bn/{case}/{q}", e, bar)
            record_parity(f"sparse_bn/{case}/{q}_torch", t, bar)
    verdict = [ln for ln in r.stdout.splitlines() if ln.startswith("BN-KNOBS-")]
    print("\n".join(verdict))
    assert r.returncode == 0 and verdict == ["BN-KNOBS-OK"], (verdict, r.stderr[-3000:])


if __name__ == "__main__":
    sys.exit(knob_child() if "--knobs" in sys.argv else 2)
