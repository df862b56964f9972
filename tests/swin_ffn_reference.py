"""The FFN half of a Swin block in float64, for the tests of `bevamd_swin_ffn_forward`: LayerNorm, Linear, erf GELU, Linear, add, on
the 16-bit inputs widened to float64.  Plain torch functions on the UNPACKED weights: no packing and no index code of the op."""
import torch
import torch.nn.functional as F


def ffn_forward(x, gamma, beta, w1, b1, w2, b2, eps):
    """x [T, C], gamma / beta [C], w1 [hidden, C], b1 [hidden], w2 [C, hidden], b2 [C] (any float dtype, host) -> float64 [T, C]."""
    x, gamma, beta, w1, b1, w2, b2 = (t.detach().cpu().double() for t in (x, gamma, beta, w1, b1, w2, b2))
    n = F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)
    t = F.linear(n, w1, b1)
    h = 0.5 * t * (1.0 + torch.erf(t / 2.0 ** 0.5))
    return x + F.linear(h, w2, b2)


def module_forward(x, norm, ffn):
    """The same from a block's `norm2` and `ffn` modules."""
    fc1, fc2 = ffn.layers[0][0], ffn.layers[1]
    return ffn_forward(x, norm.weight, norm.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, norm.eps)
