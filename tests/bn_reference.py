"""float64 reference of the training-mode BatchNorm1d (+ residual, + ReLU) kernels of csrc/sparse_bn.hip, forward and backward.

Plain torch in float64, on whatever device its arguments live on: tests/test_bn_reference.py checks it on the host against
`torch.nn.BatchNorm1d` in float64 through autograd, the GPU tests hand it device tensors so that the large cases do not cross the bus.
Nothing here calls the library.

`moments64`         mean, biased variance, invstd and the running-statistic updates from the STORED values of x.
`forward_mirror`    the kernel's forward with its rounding points, every intermediate float64, and the elementwise bound on y.
`backward_mirror`   dz, d bias, d weight, dx (rounded once) and the elementwise bound on dx, for a given mask.
`grid_facts`        how the launchers deal rows out (slabs, groups, empty slabs, grid-stride trips), from constants read in the source.
"""
import os
import re

import torch

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bevfusion_amd", "csrc", "sparse_bn.hip")

# stored mantissa bits, exponent of the smallest normal
_FORMAT = {torch.float32: (23, -126), torch.float16: (10, -14), torch.bfloat16: (7, -126)}
SLACK = 2.0 ** -20          # stands for a few fp32 roundings of the terms it multiplies


def f64(t):
    return t.detach().double()


def ulp(a, dtype):
    """Spacing of `dtype` at |a| (a float64): 2^(floor(log2 |a|) - mantissa bits), the subnormal spacing below the smallest normal."""
    mant, emin = _FORMAT[dtype]
    # by the bits of the float64, not frexp / ldexp: a device pow() need not return exact powers of two
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).contiguous()
    e = ((a.view(torch.int64) >> 52) & 0x7FF) - 1023     # floor(log2 |a|);  zero (and float64 subnormals) -> -1023 -> emin below
    e = torch.clamp(e, min=emin) - mant
    return ((e + 1023) << 52).view(torch.float64)


def round_dt(a, dtype):
    """float64 -> the nearest value of `dtype` (ties to even), still held as float64: ONE rounding, not float64 -> fp32 -> 16 bit.
    fp32 is the identity: the fp32 kernels are judged against unrounded float64."""
    if dtype == torch.float32:
        return a
    u = ulp(a, dtype)
    r = torch.round(a / u) * u                           # a / u is exact (u a power of two); torch.round: half to even
    if dtype == torch.float16:
        r = torch.where(r.abs() > 65504.0, torch.sign(r) * float("inf"), r)
    return torch.where(torch.isfinite(a), r, a)


def moments64(x, eps, momentum=None, running_mean=None, running_var=None):
    """Per-channel statistics of x [n, c] from its stored values, all float64.  Running statistics as nn.BatchNorm1d moves them:
    new = (1 - momentum) * old + momentum * (mean | unbiased variance)."""
    x = f64(x)
    n = x.shape[0]
    mean = x.mean(0)
    var = (x - mean).square().mean(0)
    out = dict(mean=mean, var=var, invstd=1.0 / torch.sqrt(var + eps), unbiased=var * (n / (n - 1.0)) if n > 1 else var)
    if momentum is not None:
        out["running_mean"] = (1.0 - momentum) * f64(running_mean) + momentum * mean
        out["running_var"] = (1.0 - momentum) * f64(running_var) + momentum * out["unbiased"]
    return out


def forward_mirror(x, mean, invstd, weight, bias, res, relu, dtype):
    """t1 = round((x - mean) * (invstd * w) + b), t2 = round(t1 + res), y = relu(t2) with the fp32 `mean` / `invstd` GIVEN (the
    kernel's own: the apply kernel is judged apart from the statistics).  `bound` is the elementwise allowance on y: one storage ulp
    of max(|t1|, |t2|) (each of the two roundings may fall the other way) + SLACK * the magnitudes that fp32 rounds on the way."""
    x, mean, invstd = f64(x), f64(mean), f64(invstd)
    w = f64(weight) if weight is not None else torch.ones_like(mean)
    b = f64(bias) if bias is not None else torch.zeros_like(mean)
    scale = invstd * w
    t1 = round_dt((x - mean) * scale + b, dtype)
    r = f64(res) if res is not None else None
    t2 = round_dt(t1 + r, dtype) if r is not None else t1
    y = torch.where(t2 <= 0, torch.zeros_like(t2), t2) if relu else t2          # NaN stays NaN
    mag = (x - mean).abs() * scale.abs() + b.abs() + (r.abs() if r is not None else 0.0)
    bound = ulp(torch.maximum(t1.abs(), t2.abs()), dtype) + SLACK * mag
    return dict(y=y, t1=t1, t2=t2, bound=bound)


def backward_mirror(x, dy, mask, mean, invstd, weight, dtype, sum_dz=None, sum_dz_xhat=None):
    """dz = mask * dy;  d bias = sum dz;  d weight = sum dz * xhat;  dx = round(w * invstd * (dz - mean(dz) - xhat * mean(dz * xhat)));
    d residual = dz.  `mask` is `~(y <= 0)` of the forward output (None: no ReLU), which is `y > 0` wherever y is a number.
    `sum_dz` / `sum_dz_xhat` (the kernel's own d bias / d weight) replace the float64 sums inside dx when given, so that the
    elementwise kernel is judged apart from the reduction.  `abs_dz` / `abs_dzx` are the scales of the two sums."""
    x, dy, mean, invstd = f64(x), f64(dy), f64(mean), f64(invstd)
    w = f64(weight) if weight is not None else torch.ones_like(mean)
    n = x.shape[0]
    dz = torch.where(mask, dy, torch.zeros_like(dy)) if mask is not None else dy
    xhat = (x - mean) * invstd
    dzx = dz * xhat
    out = dict(dz=dz, dbias=dz.sum(0), dweight=dzx.sum(0), abs_dz=dz.abs().sum(0), abs_dzx=dzx.abs().sum(0))
    m1 = (f64(sum_dz) if sum_dz is not None else out["dbias"]) / n
    m2 = (f64(sum_dz_xhat) if sum_dz_xhat is not None else out["dweight"]) / n
    k0 = w * invstd
    out["dx"] = round_dt(k0 * (dz - m1 - xhat * m2), dtype)
    out["dx_bound"] = ulp(out["dx"], dtype) + SLACK * k0.abs() * (dz.abs() + m1.abs() + (xhat * m2).abs())
    return out


def standard_inputs(dev, n, c, dtype, seed=0, with_res=True):
    """The input set of tests/test_gpu_sparse_bn.py: x ~ N(0.3, 1.7), residual and dy ~ N(0, 1) in the storage type, weight
    linspace 0.5 .. 1.5, bias linspace -0.2 .. 0.2."""
    g = torch.Generator(device=dev).manual_seed(1000003 * seed + 31 * n + c)
    x = (torch.randn((n, c), generator=g, device=dev) * 1.7 + 0.3).to(dtype)
    res = torch.randn((n, c), generator=g, device=dev).to(dtype)
    dy = torch.randn((n, c), generator=g, device=dev).to(dtype)
    return dict(x=x, res=res if with_res else None, dy=dy, weight=torch.linspace(0.5, 1.5, c, device=dev),
                bias=torch.linspace(-0.2, 0.2, c, device=dev))


def plant_relu_boundary(inputs, t1, count=200, seed=0):
    """Residual = -t1 at `count` positions (exact in the storage type), so that t1 + residual is exactly zero there.  `t1` is the
    BatchNorm output without residual and ReLU.  Returns the new input set and the flat positions."""
    g = torch.Generator(device=t1.device).manual_seed(seed)
    idx = torch.randperm(t1.numel(), generator=g, device=t1.device)[:count]
    res = inputs["res"].clone()
    res.view(-1)[idx] = -t1.detach().reshape(-1)[idx]
    return dict(inputs, res=res), idx


def source_constants(path=SRC):
    """The constants of csrc/sparse_bn.hip that decide the launch grids, read from the source so that a retune moves the edge cases of
    the tests visibly (their expected slab counts are written out next to each case)."""
    text = open(path).read()

    def one(pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0])

    return dict(threads=one(r"constexpr int THREADS = (\d+);"), group=one(r"constexpr int GROUP = (\d+);"),
                max_slabs=one(r"constexpr int MAX_SLABS = (\d+);"), default_slabs=one(r"constexpr int BN_DEFAULT_SLABS = (\d+),"),
                rows_per_lane=one(r"long long g = n / \(\(long long\)rif \* (\d+)\);"),
                apply_cap=one(r"g < 1 \? 1 : g > (\d+) \? \1 : g\);"))


def grid_facts(n, c, dtype, slabs=None, k=None):
    """What reduce_grid / apply_grid / slab_of make of n rows of c channels: `slabs` workgroups of the reducing kernels (unit =
    rows in flight * rows per lane; at most `slabs`, the default or BEVAMD_BN_SLABS), in `groups` ticket groups, `empty` trailing
    slabs that own no rows, and whether the elementwise kernels need a `second_trip` of their grid-stride loop."""
    k = k or source_constants()
    vec = 4 if dtype == torch.float32 else 8
    rif = k["threads"] // (c // vec)
    cap = min(slabs or k["default_slabs"], k["max_slabs"])
    g = min(max(n // (rif * k["rows_per_lane"]), 1), cap)
    per = -(-n // g)
    work = -(-n // (rif * 4))
    return dict(rif=rif, slabs=g, groups=-(-g // k["group"]), empty=g - (-(-n // per)), second_trip=work > k["apply_cap"])
