"""Host mirror of the camera necks' fused layer (`bevamd_neck_conv_forward`), shared by tests/test_cam_neck.py and
tests/test_gpu_cam_neck.py.  No tests here.

`resample32` is the kernel's bilinear resampling (align_corners=True) in numpy float32 with ONE operation per rounding, in exactly
the order include/bevfusion_amd_ext.h states:

    ry = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0
    sy = ry * (float)Y;  y0 = min((int)sy, h - 1);  y1 = y0 + (y0 < h - 1);  ly = sy - (float)y0;  hy = 1.f - ly      (x likewise)
    v  = hy * (hx * a[y0][x0] + lx * a[y0][x1]) + ly * (hx * a[y1][x0] + lx * a[y1][x1])

`staged` rounds v once to the storage type: that 16-bit value is the MFMA operand, bit for bit, so the float64 reference of a layer
is an ordinary convolution of the staged operands and the resampling adds nothing to the tolerance.
"""
import numpy as np
import torch
import torch.nn.functional as F


def axis_table(n, N):
    """(i0, i1, l, h) of an axis of n source and N output positions, float32 arithmetic."""
    r = np.float32(n - 1) / np.float32(N - 1) if N > 1 else np.float32(0.0)
    s = r * np.arange(N, dtype=np.float32)
    i0 = np.minimum(s.astype(np.int32), n - 1)
    i1 = i0 + (i0 < n - 1)
    l = s - i0.astype(np.float32)
    h = np.float32(1.0) - l
    assert s.dtype == l.dtype == h.dtype == np.float32
    return i0, i1, l, h


def resample32(a, out_size):
    """a: float32 array [B, C, h, w] -> float32 [B, C, H, W], every operation rounded to float32, no fused multiply-add."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    y0, y1, ly, hy = axis_table(a.shape[2], out_size[0])
    x0, x1, lx, hx = axis_table(a.shape[3], out_size[1])
    ly, hy = ly[:, None], hy[:, None]
    a00, a01 = a[:, :, y0][:, :, :, x0], a[:, :, y0][:, :, :, x1]
    a10, a11 = a[:, :, y1][:, :, :, x0], a[:, :, y1][:, :, :, x1]
    top = hx * a00 + lx * a01
    bot = hx * a10 + lx * a11
    v = hy * top + ly * bot
    assert v.dtype == np.float32
    return v


def staged(src, out_size):
    """The layer's operand from one 16-bit source: the source itself where its map is the output map (a copy), else the mirror's
    resampling rounded ONCE to the storage type."""
    src = src.detach().cpu()
    if tuple(src.shape[2:]) == tuple(out_size):
        return src
    return torch.from_numpy(resample32(src.float().numpy(), out_size)).to(src.dtype)


def ref64(srcs, w, scale, shift, kernel, relu, out_size):
    """-> (ref, mag) in float64 from the exact 16-bit operands (the staged sources and the weights) and the fp32 scale and shift:
    ref = [relu](s * conv64(x, w) + t), mag = |s| * conv64(|x|, |w|) + |t|."""
    x = torch.cat([staged(s, out_size).double() for s in srcs], dim=1)
    w = w.detach().cpu().double()
    acc = F.conv2d(x, w, padding=kernel // 2)
    mag = F.conv2d(x.abs(), w.abs(), padding=kernel // 2)
    s, t = scale.detach().cpu().double().view(1, -1, 1, 1), shift.detach().cpu().double().view(1, -1, 1, 1)
    y = s * acc + t
    return (torch.relu(y) if relu else y), s.abs() * mag + t.abs()
