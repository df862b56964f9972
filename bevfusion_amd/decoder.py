"""The learned stage of TransFusionHead on the device: the transformer decoder layer (reference:
mmdet3d/models/utils/transformer.py:14-493), its attention over csrc/ext/decoder_attention.hip.  `heads` re-exports everything here.

  * `fused_attention(q, k, v, dropout_p=0.0, seed=None)`: softmax(q k^T / 4) v per head of dimension 16 on [B, L, E] / [B, S, E]
    tensors as an autograd.Function; the [heads, L, S] logits never reach memory, forward is two launches, backward three, no host
    sync, no floating-point atomics: equal calls are bit-equal and a captured graph replays;
  * `MultiheadAttention`, `PositionEmbeddingLearned`, `TransformerDecoderLayer`: the reference's modules with its parameter names
    and shapes, so a checkpoint's `decoder.0.*` loads with strict=True; projections, LayerNorms and the FFN stay torch ops in the
    reference's order.

There is no CPU path: host tensors raise.  `_attention_host`, `_dropout_keep_host` and `_layer_host` restate the arithmetic on the
host for the tests.

Differences from the reference, on purpose: the projection branch is chosen by object identity (`key is value`, `query is key`), not
by two `torch.equal` calls: all three branches slice `in_proj_weight` the same way, so the result is the same and two device-to-host
syncs are gone; `need_weights` defaults to False and the head-averaged weights are not served (the layer discards them);
attention dropout is a counter hash of (seed, head, query, key) with the seed drawn from torch's CPU generator, not torch's device
generator: `torch.manual_seed` reproduces a step, the mask differs from the reference's; fp16 inputs run the fp16 forward only when
no gradient is needed and are upcast to fp32 for forward and backward otherwise (the backward kernel is fp32); attn_mask,
key_padding_mask, add_bias_kv, add_zero_attn, kdim / vdim and static_k / static_v raise NotImplementedError (no config uses them).

The C ABI goes beyond the three entry points first specified for it: `bevamd_mha_forward` also writes `stats` [2, B, H, L] (lse
in two terms, which `bevamd_mha_backward` reads in place of lse: at logits near 96 an fp32 lse has an ulp of 7.6e-6), both take the
workspace size like every other entry point, and `bevamd_mha_plan` (`attention_plan` here) reports the split and block counts of a
shape, so tests can build shapes on the kernels' own constants.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi

__all__ = ["fused_attention", "attention_plan", "MultiheadAttention", "PositionEmbeddingLearned", "TransformerDecoderLayer",
           "HEAD_DIM", "MAX_HEADS", "MAX_QUERIES", "MAX_KEYS", "SPLIT_KEYS_MIN", "BACKWARD_BLOCK_KEYS"]

HEAD_DIM = 16                 # MH_D of the kernels, the only head dimension
MAX_HEADS = 16
MAX_QUERIES = 1024
MAX_KEYS = 1 << 20
SPLIT_KEYS_MIN = 64           # MH_KSTEP: a forward split is a multiple of it
BACKWARD_BLOCK_KEYS = 256     # MH_BWD_KEYS: a backward key block is a multiple of it


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("the decoder attention needs GPU tensors (there is no CPU path)")


def attention_plan(B, H, L, S):
    """(forward splits, keys per split, backward key blocks, keys per block) of a shape: functions of (B, H, L, S) alone."""
    plan = (ctypes.c_int * 4)()
    _capi.check(_capi.load().bevamd_mha_plan(int(B), int(H), int(L), int(S), plan), "mha_plan")
    return tuple(plan)


def _check_shapes(q, k, v):
    if q.dim() != 3 or k.dim() != 3 or v.shape != k.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]:
        raise RuntimeError(f"q [B, L, E], k and v [B, S, E] expected, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    B, L, E = q.shape
    S = k.shape[1]
    if E % HEAD_DIM:
        raise ValueError(f"embedding of {E}: heads of dimension {HEAD_DIM} only")
    H = E // HEAD_DIM
    if not (1 <= H <= MAX_HEADS and 1 <= L <= MAX_QUERIES and 1 <= S <= MAX_KEYS and B >= 1):
        raise ValueError(f"B {B}, {H} heads (1 .. {MAX_HEADS}), {L} queries (1 .. {MAX_QUERIES}), {S} keys (1 .. {MAX_KEYS})")
    return B, H, L, S


def _dense(t):
    """Contiguous and 16-byte aligned (the kernels load 16 bytes at a time): a copy where the tensor is neither."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _workspace(B, H, L, S, dev):
    size = _capi.load().bevamd_mha_workspace_bytes(B, H, L, S)
    if size == 0:
        raise ValueError(f"attention shape B {B}, H {H}, L {L}, S {S} is not served")
    return torch.empty(size, dtype=torch.uint8, device=dev), size


def _forward(q, k, v, p, seed, want_stats=False):
    """q, k, v contiguous fp32 | fp16 on one device -> (out, lse [B, H, L] fp32, stats [2, B, H, L] fp32 or None: lse in two terms,
    the row maximum and the log of the row sum, for the backward)."""
    B, H, L, S = _check_shapes(q, k, v)
    dev = q.device
    out = torch.empty_like(q)
    lse = torch.empty((B, H, L), dtype=torch.float32, device=dev)
    stats = torch.empty((2, B, H, L), dtype=torch.float32, device=dev) if want_stats else None
    ws, size = _workspace(B, H, L, S, dev)
    with torch.cuda.device(dev):
        rc = _capi.load().bevamd_mha_forward(_capi.ptr(q), _capi.ptr(k), _capi.ptr(v), B, H, L, S, 0 if q.dtype == torch.float32 else 1,
                                             float(p), int(seed), _capi.ptr(out), _capi.ptr(lse), _capi.ptr(stats), _capi.ptr(ws), size,
                                             _capi.stream_ptr(dev))
    _capi.check(rc, "mha_forward")
    return out, lse, stats


class _FusedAttention(torch.autograd.Function):
    """q, k, v dense fp32.  The backward is not differentiable again (once_differentiable: a double backward raises)."""

    @staticmethod
    def forward(ctx, q, k, v, p, seed):
        out, _, stats = _forward(q, k, v, p, seed, want_stats=True)
        ctx.save_for_backward(q, k, v, out, stats)
        ctx.p, ctx.seed = p, seed
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, out, stats = ctx.saved_tensors
        B, H, L, S = _check_shapes(q, k, v)
        dev = q.device
        dout = _dense(dout)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws, size = _workspace(B, H, L, S, dev)
        with torch.cuda.device(dev):
            rc = _capi.load().bevamd_mha_backward(_capi.ptr(q), _capi.ptr(k), _capi.ptr(v), _capi.ptr(out), _capi.ptr(stats),
                                                  _capi.ptr(dout), B, H, L, S, float(ctx.p), int(ctx.seed), _capi.ptr(dq), _capi.ptr(dk),
                                                  _capi.ptr(dv), _capi.ptr(ws), size, _capi.stream_ptr(dev))
        _capi.check(rc, "mha_backward")
        return dq, dk, dv, None, None


def fused_attention(q, k, v, dropout_p=0.0, seed=None, return_lse=False):
    """q [B, L, E], k, v [B, S, E] on the device, fp32 or fp16, E = heads * 16 -> [B, L, E]: per head softmax(q k^T / 4) v, the
    softmax and both sums in fp32.  dropout_p > 0 drops normalised weights by the counter hash of (seed, b * H + h, query, key)
    (`_dropout_keep_host`) and scales the kept ones by 1 / (1 - p); seed None draws one from torch's CPU generator.  Differentiable
    in q, k, v (fp16 inputs are then computed in fp32 and the result cast back).  return_lse (no gradient): also the [B, H, L] fp32
    log-sum-exp of the scaled logits.  No host sync."""
    _need_gpu(q, k, v)
    if q.dtype not in (torch.float32, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise RuntimeError(f"q, k, v must share float32 or float16, got {q.dtype}, {k.dtype}, {v.dtype}")
    if not 0.0 <= float(dropout_p) < 1.0:
        raise ValueError(f"dropout_p {dropout_p} (0 <= p < 1)")
    _check_shapes(q, k, v)
    if dropout_p > 0.0 and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())        # the CPU generator: no device sync
    seed = 0 if seed is None else int(seed) & (2 ** 64 - 1)
    grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)
    if return_lse:
        return _forward(_dense(q.detach()), _dense(k.detach()), _dense(v.detach()), float(dropout_p), seed)[:2]
    if not grad:
        return _forward(_dense(q.detach()), _dense(k.detach()), _dense(v.detach()), float(dropout_p), seed)[0]
    dtype = q.dtype
    out = _FusedAttention.apply(_dense(q.float()), _dense(k.float()), _dense(v.float()), float(dropout_p), seed)
    return out.to(dtype)


# ---- modules ---------------------------------------------------------------------------------------------------------------------
class PositionEmbeddingLearned(nn.Module):
    """transformer.py:14-30: [B, P, input_channel] positions -> [B, num_pos_feats, P]."""

    def __init__(self, input_channel, num_pos_feats=288):
        super().__init__()
        self.position_embedding_head = nn.Sequential(
            nn.Conv1d(input_channel, num_pos_feats, kernel_size=1), nn.BatchNorm1d(num_pos_feats), nn.ReLU(inplace=True),
            nn.Conv1d(num_pos_feats, num_pos_feats, kernel_size=1))

    def forward(self, xyz):
        return self.position_embedding_head(xyz.transpose(1, 2).contiguous())


class MultiheadAttention(nn.Module):
    """transformer.py:114-241 over `fused_attention`: (L, N, E) query, (S, N, E) key and value -> ((L, N, E), None)."""

    def __init__(self, embed_dim, num_heads, dropout=0., bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None, vdim=None):
        super().__init__()
        if add_bias_kv:
            raise NotImplementedError("add_bias_kv is not served")
        if add_zero_attn:
            raise NotImplementedError("add_zero_attn is not served")
        if (kdim is not None and kdim != embed_dim) or (vdim is not None and vdim != embed_dim):
            raise NotImplementedError("kdim / vdim different from embed_dim are not served")
        if embed_dim % num_heads or embed_dim // num_heads != HEAD_DIM:
            raise ValueError(f"embed_dim {embed_dim} over {num_heads} heads: the head dimension must be {HEAD_DIM}")
        self.embed_dim, self.kdim, self.vdim = embed_dim, embed_dim, embed_dim
        self.num_heads, self.dropout, self.head_dim = num_heads, dropout, HEAD_DIM
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        if bias:
            self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.bias_k = self.bias_v = None
        self.add_zero_attn = False
        self._reset_parameters()

    def _reset_parameters(self):
        nn.init.xavier_uniform_(self.in_proj_weight)
        if self.in_proj_bias is not None:
            nn.init.constant_(self.in_proj_bias, 0.)
            nn.init.constant_(self.out_proj.bias, 0.)

    def forward(self, query, key, value, key_padding_mask=None, need_weights=False, attn_mask=None, static_k=None, static_v=None):
        if need_weights:
            raise NotImplementedError("need_weights=True is not served: the attention weights are never materialised")
        if attn_mask is not None:
            raise NotImplementedError("attn_mask is not served")
        if key_padding_mask is not None:
            raise NotImplementedError("key_padding_mask is not served")
        if static_k is not None or static_v is not None:
            raise NotImplementedError("static_k / static_v are not served")
        _need_gpu(query, key, value)
        E = self.embed_dim
        if query.dim() != 3 or query.shape[2] != E or key.shape != value.shape or key.shape[1:] != query.shape[1:]:
            raise RuntimeError(f"query (L, N, {E}), key and value (S, N, {E}) expected, got {tuple(query.shape)}, {tuple(key.shape)}, "
                               f"{tuple(value.shape)}")
        w, b = self.in_proj_weight, self.in_proj_bias

        def part(lo, hi):
            return w[lo:hi], None if b is None else b[lo:hi]

        if key is value and query is key:                                  # self-attention: one projection
            q, k, v = F.linear(query, w, b).chunk(3, dim=-1)
        elif key is value:                                                 # encoder-decoder attention: key and value share one
            q = F.linear(query, *part(0, E))
            k, v = F.linear(key, *part(E, 3 * E)).chunk(2, dim=-1)
        else:
            q, k, v = F.linear(query, *part(0, E)), F.linear(key, *part(E, 2 * E)), F.linear(value, *part(2 * E, 3 * E))
        p = float(self.dropout) if self.training else 0.0
        out = fused_attention(q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1), dropout_p=p)      # [N, L, E]
        return self.out_proj(out.transpose(0, 1)), None


def _activation(name):
    if name == "relu":
        return F.relu
    if name == "gelu":
        return F.gelu
    if name == "glu":
        return F.glu
    raise RuntimeError(f"activation should be relu/gelu, not {name}.")


class TransformerDecoderLayer(nn.Module):
    """transformer.py:33-111: query [B, C, Pq], key [B, C, Pk], positions [B, P, 2 | 3 | 6] -> [B, C, Pq]."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", self_posembed=None, cross_posembed=None,
                 cross_only=False):
        super().__init__()
        self.cross_only = cross_only
        if not self.cross_only:
            self.self_attn = MultiheadAttention(d_model, nhead, dropout=dropout)
        self.multihead_attn = MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.dropout3 = nn.Dropout(dropout)
        self.activation = _activation(activation)
        self.self_posembed = self_posembed
        self.cross_posembed = cross_posembed

    def with_pos_embed(self, tensor, pos_embed):
        return tensor if pos_embed is None else tensor + pos_embed

    def forward(self, query, key, query_pos, key_pos, attn_mask=None):
        if attn_mask is not None:
            raise NotImplementedError("attn_mask is not served")
        _need_gpu(query, key, query_pos, key_pos)
        query_pos_embed = self.self_posembed(query_pos).permute(2, 0, 1) if self.self_posembed is not None else None
        key_pos_embed = self.cross_posembed(key_pos).permute(2, 0, 1) if self.cross_posembed is not None else None
        query = query.permute(2, 0, 1)
        key = key.permute(2, 0, 1)
        if not self.cross_only:
            q = k = v = self.with_pos_embed(query, query_pos_embed)
            query2 = self.self_attn(q, k, value=v)[0]
            query = query + self.dropout1(query2)
            query = self.norm1(query)
        kv = self.with_pos_embed(key, key_pos_embed)                       # one tensor for key and value: one projection
        query2 = self.multihead_attn(query=self.with_pos_embed(query, query_pos_embed), key=kv, value=kv)[0]
        query = query + self.dropout2(query2)
        query = self.norm2(query)
        query2 = self.linear2(self.dropout(self.activation(self.linear1(query))))
        query = query + self.dropout3(query2)
        query = self.norm3(query)
        return query.permute(1, 2, 0)


# ---- host mirrors (tests only) ---------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _mix64(z):
    z = (z + np.uint64(0x9E3779B97F4A7C15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _dropout_keep_host(seed, B, H, L, S, p):
    """The kernels' dropout mask: bool [B, H, L, S], True where the weight is kept."""
    with np.errstate(over="ignore"):
        rows = (np.arange(B * H, dtype=np.uint64)[:, None] << np.uint64(10)) | np.arange(L, dtype=np.uint64)[None, :]
        z = _mix64(_mix64(np.array([int(seed) & _M64], dtype=np.uint64)) + rows)                    # [BH, L]
        lo = (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, :, None]
        hi = (z >> np.uint64(32)).astype(np.uint32)[:, :, None]
        x = np.arange(S, dtype=np.uint32)[None, None, :] * np.uint32(0x9E3779B1) + lo
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x += hi
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
    threshold = min(int(float(p) * 4294967296.0), 4294967295)
    return (x >= np.uint32(threshold)).reshape(B, H, L, S)


def _attention_host(q, k, v, keep=None, p=0.0, return_lse=False):
    """numpy float64: q [B, L, E], k, v [B, S, E] -> [B, L, E] (and lse [B, H, L]); keep: bool [B, H, L, S] of kept weights."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    B, L, E = q.shape
    S, H = k.shape[1], E // HEAD_DIM
    qh = q.reshape(B, L, H, HEAD_DIM).transpose(0, 2, 1, 3) * 0.25
    kh = k.reshape(B, S, H, HEAD_DIM).transpose(0, 2, 1, 3)
    vh = v.reshape(B, S, H, HEAD_DIM).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    total = e.sum(-1, keepdims=True)
    w = e / total
    if keep is not None:
        w = np.where(keep, w / (1.0 - p), 0.0)
    out = (w @ vh).transpose(0, 2, 1, 3).reshape(B, L, E)
    if return_lse:
        return out, (m + np.log(total))[..., 0]
    return out


def _attention_torch(q, k, v, keep=None, p=0.0):
    """The reference's formulation (bmm, softmax, bmm) on torch tensors of any dtype and device, differentiable."""
    B, L, E = q.shape
    S, H = k.shape[1], E // HEAD_DIM
    qh = (q * 0.25).reshape(B, L, H, HEAD_DIM).permute(0, 2, 1, 3).reshape(B * H, L, HEAD_DIM)
    kh = k.reshape(B, S, H, HEAD_DIM).permute(0, 2, 1, 3).reshape(B * H, S, HEAD_DIM)
    vh = v.reshape(B, S, H, HEAD_DIM).permute(0, 2, 1, 3).reshape(B * H, S, HEAD_DIM)
    w = torch.softmax(torch.bmm(qh, kh.transpose(1, 2)), dim=-1)
    if keep is not None:
        w = torch.where(keep.reshape(B * H, L, S), w / (1.0 - p), torch.zeros_like(w))
    return torch.bmm(w, vh).reshape(B, H, L, HEAD_DIM).permute(0, 2, 1, 3).reshape(B, L, E)


def _layer_host(state_dict, query, key, query_pos, key_pos, nhead=8, cross_only=False, activation="relu", eps=1e-5, attention=None,
                training=False):
    """The layer in eval mode, or (training=True) in train mode with all dropouts 0: BatchNorm on batch statistics, in CPU torch
    float64 with autograd.  state_dict: the layer's (tensors or arrays; float64 host tensors are used as they are, so gradients
    reach those that require them); query [B, C, Pq], key [B, C, Pk], positions [B, P, D] tensors or arrays.  attention(q, k, v) on
    [B, L, E] tensors replaces the float64 attention.  -> [B, C, Pq]."""
    def t(x):
        if isinstance(x, torch.Tensor):
            return x if x.dtype == torch.float64 and not x.is_cuda else x.detach().cpu().double()
        return torch.from_numpy(np.asarray(x, np.float64))

    sd = {name: t(value) for name, value in state_dict.items() if not name.endswith("num_batches_tracked")}
    attention = attention or _attention_torch
    act = _activation(activation)

    def posembed(prefix, xyz):
        if prefix + ".position_embedding_head.0.weight" not in sd:
            return None
        g = lambda n: sd[f"{prefix}.position_embedding_head.{n}"]
        x = F.conv1d(t(xyz).transpose(1, 2), g("0.weight"), g("0.bias"))
        if training:
            x = F.batch_norm(x, None, None, g("1.weight"), g("1.bias"), True, 0.0, eps)
        else:
            x = F.batch_norm(x, g("1.running_mean"), g("1.running_var"), g("1.weight"), g("1.bias"), False, 0.0, eps)
        return F.conv1d(F.relu(x), g("3.weight"), g("3.bias")).permute(2, 0, 1)

    def mha(prefix, q_in, kv_in):
        w, b = sd[prefix + ".in_proj_weight"], sd[prefix + ".in_proj_bias"]
        E = w.shape[1]
        q = F.linear(q_in, w[:E], b[:E])
        k, v = F.linear(kv_in, w[E:], b[E:]).chunk(2, dim=-1)
        out = attention(q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1)).transpose(0, 1)
        return F.linear(out, sd[prefix + ".out_proj.weight"], sd[prefix + ".out_proj.bias"])

    def norm(prefix, x):
        return F.layer_norm(x, (x.shape[-1],), sd[prefix + ".weight"], sd[prefix + ".bias"], eps)

    def add(x, pos):
        return x if pos is None else x + pos

    qpos, kpos = posembed("self_posembed", query_pos), posembed("cross_posembed", key_pos)
    x, mem = t(query).permute(2, 0, 1), t(key).permute(2, 0, 1)
    if not cross_only:
        qk = add(x, qpos)
        x = norm("norm1", x + mha("self_attn", qk, qk))
    x = norm("norm2", x + mha("multihead_attn", add(x, qpos), add(mem, kpos)))
    x = norm("norm3", x + F.linear(act(F.linear(x, sd["linear1.weight"], sd["linear1.bias"])), sd["linear2.weight"], sd["linear2.bias"]))
    return x.permute(1, 2, 0)
