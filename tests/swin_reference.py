"""A float64 restatement of mmdet 2.x's Swin Transformer written the long way: `F.pad`, `torch.roll`, window partition, a mask tensor
built with the slice loops, `softmax`, window reverse, roll back, crop.  It shares no index arithmetic with
bevfusion_amd/csrc/ext/window_attention.hip (which never forms a rolled, partitioned or padded tensor) and no code with
bevfusion_amd/cam_swin.py: the modules' weights are read from a state dict by their mmdet names.

  shifted_window_attention   the attention between the qkv Linear and the proj Linear, from a qkv map (what the kernel computes);
                             also returns mag = sum_j p_j |v_j| and row_max = max_j (scale * sum_d |q_d| |k_jd| + |bias_j|) of the query's row, which the
                             GPU test's error bar is made of
  swin_forward               the whole backbone from a state dict
"""
import math

import torch
import torch.nn.functional as F


def _partition(x, ws):
    B, H, W, C = x.shape
    x = x.reshape(B, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def _reverse(windows, ws, B, H, W):
    x = windows.reshape(B, H // ws, W // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, -1)


def region_map(Hp, Wp, ws, shift):
    """[Hp, Wp] int: the region count of mmdet's img_mask in the rolled frame."""
    img = torch.zeros(Hp, Wp, dtype=torch.int64)
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[h, w] = cnt
            cnt += 1
    return img


def shifted_window_attention(qkv, pad_qkv, bias, scale, shift, heads, ws=7):
    """qkv [B, H, W, 3C] float64 (channel which * C + head * hd + d), pad_qkv [3C] float64 (the q, k, v of a padded token) or None,
    bias [heads, ws^2, ws^2] float64.  -> (out, mag, row_max), each [B, H, W, C]; row_max is constant over a head's channels."""
    qkv = qkv.double()
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    N = ws * ws
    pad_b, pad_r = (ws - H % ws) % ws, (ws - W % ws) % ws
    Hp, Wp = H + pad_b, W + pad_r
    padded = torch.zeros(B, Hp, Wp, C3, dtype=torch.float64)
    if pad_qkv is not None:
        padded[:] = pad_qkv.double()
    padded[:, :H, :W] = qkv
    mask = None
    if shift > 0:
        padded = torch.roll(padded, shifts=(-shift, -shift), dims=(1, 2))
        mw = _partition(region_map(Hp, Wp, ws, shift).reshape(1, Hp, Wp, 1).double(), ws).reshape(-1, N)
        mask = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = torch.where(mask != 0, torch.full_like(mask, -100.0), torch.zeros_like(mask))      # [nW, N, N]
    win = _partition(padded, ws)                                                       # [B nW, N, 3C]
    BW = win.shape[0]
    win = win.reshape(BW, N, 3, heads, hd).permute(2, 0, 3, 1, 4)                      # [3, B nW, heads, N, hd]
    q, k, v = win[0], win[1], win[2]
    logits = scale * (q @ k.transpose(-2, -1)) + bias.double().unsqueeze(0)
    row = (scale * (q.abs() @ k.abs().transpose(-2, -1)) + bias.double().abs().unsqueeze(0)).max(dim=-1, keepdim=True).values
    if mask is not None:
        nW = mask.shape[0]
        logits = (logits.reshape(BW // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).reshape(BW, heads, N, N)
    p = torch.softmax(logits, dim=-1)
    outs = []
    for val in (p @ v, p @ v.abs(), row.expand(BW, heads, N, hd)):
        x = _reverse(val.transpose(1, 2).reshape(BW, N, C), ws, B, Hp, Wp)
        if shift > 0:
            x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
        outs.append(x[:, :H, :W].contiguous())
    return outs[0], outs[1], outs[2]


def _ln(x, sd, prefix):
    return F.layer_norm(x, (x.shape[-1],), sd[prefix + ".weight"], sd[prefix + ".bias"], 1e-5)


def _lin(x, sd, prefix):
    return F.linear(x, sd[prefix + ".weight"], sd.get(prefix + ".bias"))


def _corner(x, k, s):
    H, W = x.shape[-2:]
    ph = max((math.ceil(H / s) - 1) * s + k - H, 0)
    pw = max((math.ceil(W / s) - 1) * s + k - W, 0)
    return F.pad(x, (0, pw, 0, ph))


def patch_merging(x, hw, sd, prefix):
    """x [B, L, C] -> ([B, L', 2C], (H', W')): 2 x 2 neighbours gathered by hand in nn.Unfold's channel order c * 4 + ky * 2 + kx."""
    B, L, C = x.shape
    H, W = hw
    m = _corner(x.reshape(B, H, W, C).permute(0, 3, 1, 2), 2, 2)
    H2, W2 = m.shape[2] // 2, m.shape[3] // 2
    g = torch.zeros(B, H2, W2, C, 2, 2, dtype=x.dtype)
    for ky in range(2):
        for kx in range(2):
            g[..., ky, kx] = m[:, :, ky::2, kx::2].permute(0, 2, 3, 1)
    g = g.reshape(B, H2 * W2, C * 4)
    return _lin(_ln(g, sd, prefix + ".norm"), sd, prefix + ".reduction"), (H2, W2)


def swin_block(x, hw, sd, prefix, heads, shift, ws=7):
    B, L, C = x.shape
    H, W = hw
    h = _ln(x, sd, prefix + ".norm1")
    w = prefix + ".attn.w_msa"
    qkv = _lin(h, sd, w + ".qkv").reshape(B, H, W, 3 * C)
    pad = sd.get(w + ".qkv.bias")                       # the qkv of a zero token
    N = ws * ws
    bias = sd[w + ".relative_position_bias_table"][sd[w + ".relative_position_index"].reshape(-1).long()]
    bias = bias.reshape(N, N, heads).permute(2, 0, 1)
    a, _, _ = shifted_window_attention(qkv, pad, bias, (C // heads) ** -0.5, shift, heads, ws)
    x = x + _lin(a.reshape(B, L, C), sd, w + ".proj")
    f = prefix + ".ffn.layers"
    return x + _lin(F.gelu(_lin(_ln(x, sd, prefix + ".norm2"), sd, f + ".0.0")), sd, f + ".1")


def swin_forward(sd, img, depths, num_heads, out_indices, patch=4, ws=7):
    """The backbone in float64 from a state dict with mmdet's keys.  -> list of [B, C_i, H_i, W_i] for i in out_indices."""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x = F.conv2d(_corner(img.double(), patch, patch), sd["patch_embed.projection.weight"], sd["patch_embed.projection.bias"], stride=patch)
    hw = (x.shape[2], x.shape[3])
    x = x.flatten(2).transpose(1, 2)
    if "patch_embed.norm.weight" in sd:
        x = _ln(x, sd, "patch_embed.norm")
    outs = []
    for i, depth in enumerate(depths):
        for j in range(depth):
            x = swin_block(x, hw, sd, f"stages.{i}.blocks.{j}", num_heads[i], ws // 2 if j % 2 else 0, ws)
        if i in out_indices:
            o = _ln(x, sd, f"norm{i}")
            outs.append(o.reshape(-1, hw[0], hw[1], o.shape[-1]).permute(0, 3, 1, 2).contiguous())
        if i < len(depths) - 1:
            x, hw = patch_merging(x, hw, sd, f"stages.{i}.downsample")
    return outs
