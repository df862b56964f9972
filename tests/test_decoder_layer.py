"""CPU: the decoder layer's host mirrors against the reference's recorded float64 outputs, its state dict, argument rejection and
the dropout hash (tests/golden/decoder_layer_ref.npz, written by tests/golden/make_decoder_layer_golden.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi, decoder, heads

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_decoder_layer_golden", os.path.join(HERE, "golden", "make_decoder_layer_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


MAKER = _load_maker()
GOLDEN = np.load(os.path.join(HERE, "golden", "decoder_layer_ref.npz"))
TAGS = {False: "full", True: "cross_only"}


def _posembed():
    return decoder.PositionEmbeddingLearned(MAKER.POS_DIM, MAKER.D_MODEL)


def _layer(cross_only=False, dropout=0.1):
    return decoder.TransformerDecoderLayer(MAKER.D_MODEL, MAKER.HEADS, MAKER.FFN_DIM, dropout=dropout, self_posembed=_posembed(),
                                           cross_posembed=_posembed(), cross_only=cross_only)


@pytest.mark.parametrize("cross_only", [False, True])
def test_golden_inputs_are_the_recorded_ones(cross_only):
    assert MAKER.digest(cross_only) == str(GOLDEN[f"{TAGS[cross_only]}.inputs_sha256"])


@pytest.mark.parametrize("cross_only", [False, True])
def test_attention_host_reproduces_the_reference(cross_only):
    """The reference's multi_head_attention_forward in float64 on the cross-attention's own inputs: projections in numpy, the
    attention by `_attention_host`."""
    tag = TAGS[cross_only]
    w = {k: v.astype(np.float64) for k, v in MAKER.layer_weights(cross_only).items()}
    E = MAKER.D_MODEL
    x, mem = GOLDEN[f"{tag}.attn_query64"], GOLDEN[f"{tag}.attn_key64"]                      # (L, N, E), (S, N, E)
    wi, bi = w["multihead_attn.in_proj_weight"], w["multihead_attn.in_proj_bias"]
    q = x @ wi[:E].T + bi[:E]
    k = mem @ wi[E:2 * E].T + bi[E:2 * E]
    v = mem @ wi[2 * E:].T + bi[2 * E:]
    out = decoder._attention_host(q.transpose(1, 0, 2), k.transpose(1, 0, 2), v.transpose(1, 0, 2)).transpose(1, 0, 2)
    out = out @ w["multihead_attn.out_proj.weight"].T + w["multihead_attn.out_proj.bias"]
    want = GOLDEN[f"{tag}.attn_out64"]
    assert out.shape == want.shape and np.abs(out - want).max() <= 1e-12


@pytest.mark.parametrize("cross_only", [False, True])
def test_layer_host_reproduces_the_reference(cross_only):
    out = decoder._layer_host(MAKER.layer_weights(cross_only), *MAKER.case_inputs(), nhead=MAKER.HEADS, cross_only=cross_only)
    want = GOLDEN[f"{TAGS[cross_only]}.out64"]
    assert out.dtype == torch.float64 and tuple(out.shape) == want.shape
    assert np.abs(out.numpy() - want).max() <= 1e-12


def test_layer_host_with_the_numpy_attention_agrees():
    """`_layer_host` with `_attention_host` as its attention: the two mirrors are one arithmetic."""
    def attention(q, k, v):
        return torch.from_numpy(decoder._attention_host(q.numpy(), k.numpy(), v.numpy()))

    out = decoder._layer_host(MAKER.layer_weights(), *MAKER.case_inputs(), nhead=MAKER.HEADS, attention=attention)
    assert np.abs(out.numpy() - GOLDEN["full.out64"]).max() <= 1e-12


@pytest.mark.parametrize("cross_only", [False, True])
def test_state_dict_has_the_reference_names_and_shapes(cross_only):
    tag = TAGS[cross_only]
    layer = _layer(cross_only)
    state = layer.state_dict()
    assert list(state) == [str(n) for n in GOLDEN[f"{tag}.names"]]
    assert [",".join(str(d) for d in v.shape) for v in state.values()] == [str(s) for s in GOLDEN[f"{tag}.shapes"]]
    assert len(state) == (32 if cross_only else 36)
    fresh = {str(n): torch.from_numpy(np.asarray(MAKER.layer_weights(cross_only)[str(n)])) for n in GOLDEN[f"{tag}.names"]}
    result = layer.load_state_dict(fresh, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(layer.multihead_attn.in_proj_weight.detach(), fresh["multihead_attn.in_proj_weight"])


def test_reset_parameters_is_the_reference_initialisation():
    torch.manual_seed(3)
    attn = decoder.MultiheadAttention(128, 8)
    bound = (6.0 / (384 + 128)) ** 0.5
    w = attn.in_proj_weight.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound and abs(float(w.mean())) < 0.01
    assert float(attn.in_proj_bias.detach().abs().max()) == 0.0 and float(attn.out_proj.bias.detach().abs().max()) == 0.0
    assert decoder.MultiheadAttention(32, 2, bias=False).in_proj_bias is None
    assert heads.TransformerDecoderLayer is decoder.TransformerDecoderLayer and heads.fused_attention is decoder.fused_attention


def test_host_tensors_raise():
    q, k = torch.zeros(1, 4, 128), torch.zeros(1, 9, 128)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        decoder.fused_attention(q, k, k)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        decoder.MultiheadAttention(128, 8)(q.transpose(0, 1), k.transpose(0, 1), k.transpose(0, 1))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        _layer()(torch.zeros(1, 128, 4), torch.zeros(1, 128, 9), torch.zeros(1, 4, 2), torch.zeros(1, 9, 2))


def test_unsupported_options_raise_by_name():
    for kwargs, name in ((dict(add_bias_kv=True), "add_bias_kv"), (dict(add_zero_attn=True), "add_zero_attn"), (dict(kdim=64), "kdim"),
                         (dict(vdim=64), "vdim")):
        with pytest.raises(NotImplementedError, match=name):
            decoder.MultiheadAttention(128, 8, **kwargs)
    assert decoder.MultiheadAttention(128, 8, kdim=128, vdim=128).kdim == 128
    attn = decoder.MultiheadAttention(128, 8)
    x = torch.zeros(3, 1, 128)
    for kwargs, name in ((dict(need_weights=True), "need_weights"), (dict(attn_mask=torch.zeros(3, 3)), "attn_mask"),
                         (dict(key_padding_mask=torch.zeros(1, 3, dtype=torch.bool)), "key_padding_mask"),
                         (dict(static_k=torch.zeros(8, 3, 16)), "static_k"), (dict(static_v=torch.zeros(8, 3, 16)), "static_v")):
        with pytest.raises(NotImplementedError, match=name):
            attn(x, x, x, **kwargs)
    with pytest.raises(NotImplementedError, match="attn_mask"):
        _layer()(torch.zeros(1, 128, 4), torch.zeros(1, 128, 9), torch.zeros(1, 4, 2), torch.zeros(1, 9, 2), attn_mask=torch.zeros(4, 9))


def test_head_dimension_other_than_16_raises():
    for embed, nhead in ((128, 4), (128, 16), (64, 8), (120, 8)):
        with pytest.raises(ValueError, match="head dimension"):
            decoder.MultiheadAttention(embed, nhead)
    with pytest.raises(ValueError, match="head dimension"):
        decoder.TransformerDecoderLayer(256, 8)


def test_workspace_query_rejects_what_the_entry_points_reject():
    lib = _capi.load()
    assert lib.bevamd_mha_workspace_bytes(1, 17, 200, 32400) == 0
    assert lib.bevamd_mha_workspace_bytes(1, 8, 1025, 32400) == 0
    assert lib.bevamd_mha_workspace_bytes(1, 8, 200, 0) == 0
    assert lib.bevamd_mha_workspace_bytes(0, 8, 200, 32400) == 0 and lib.bevamd_mha_workspace_bytes(1, 8, 200, (1 << 20) + 1) == 0
    assert lib.bevamd_mha_workspace_bytes(1, 8, 200, 32400) > 0 and lib.bevamd_mha_workspace_bytes(1, 16, 1024, 1 << 20) > 0
    # the entry points themselves: an error string before any GPU work (null pointers are never touched)
    rc = lib.bevamd_mha_forward(None, None, None, 1, 17, 200, 32400, 0, 0.0, 0, None, None, None, None, 0, None)
    assert rc == 1 and "bad sizes" in _capi.last_error()
    rc = lib.bevamd_mha_backward(None, None, None, None, None, None, 1, 8, 1025, 100, 0.0, 0, None, None, None, None, 0, None)
    assert rc == 1 and "bad sizes" in _capi.last_error()
    rc = lib.bevamd_mha_forward(None, None, None, 1, 8, 200, 32400, 2, 0.0, 0, None, None, None, None, 0, None)
    assert rc == 4 and "dtype" in _capi.last_error()
    rc = lib.bevamd_mha_forward(None, None, None, 1, 8, 200, 32400, 0, 1.0, 0, None, None, None, None, 0, None)
    assert rc == 1 and "dropout_p" in _capi.last_error()
    rc = lib.bevamd_mha_forward(None, None, None, 1, 8, 200, 32400, 0, 0.0, 0, None, None, None, None, 0, None)
    assert rc == 1 and "null pointer" in _capi.last_error()


def test_split_plan_is_a_function_of_the_shape():
    splits, split_keys, blocks, block_keys = decoder.attention_plan(1, 8, 200, 32400)
    assert split_keys % decoder.SPLIT_KEYS_MIN == 0 and (splits - 1) * split_keys < 32400 <= splits * split_keys and splits > 1
    assert block_keys % decoder.BACKWARD_BLOCK_KEYS == 0 and (blocks - 1) * block_keys < 32400 <= blocks * block_keys
    assert decoder.attention_plan(1, 8, 200, 32400) == (splits, split_keys, blocks, block_keys)
    assert decoder.attention_plan(1, 1, 1, decoder.SPLIT_KEYS_MIN)[:2] == (1, decoder.SPLIT_KEYS_MIN)
    assert decoder.attention_plan(1, 1, 1, decoder.SPLIT_KEYS_MIN + 1)[:2] == (2, decoder.SPLIT_KEYS_MIN)
    for shape in ((8, 8, 200, 32400), (1, 16, 1024, 1 << 20), (3, 2, 15, 17)):
        s, sk, b, bk = decoder.attention_plan(*shape)
        assert (s - 1) * sk < shape[3] <= s * sk and (b - 1) * bk < shape[3] <= b * bk


def test_dropout_hash():
    B, H, L, S, p = 1, 8, 200, 4096, 0.1
    keep = decoder._dropout_keep_host(11, B, H, L, S, p)
    assert keep.shape == (B, H, L, S) and keep.dtype == np.bool_
    assert np.array_equal(keep, decoder._dropout_keep_host(11, B, H, L, S, p))
    other = decoder._dropout_keep_host(12, B, H, L, S, p)
    assert 0.1 < (keep != other).mean() < 0.26                              # independent masks differ at 2 p (1 - p) = 0.18
    sd = lambda n: np.sqrt(p * (1 - p) / n)
    assert abs(keep.mean() - (1 - p)) <= 5 * sd(keep.size)
    assert np.abs(keep.mean(axis=(0, 2, 3)) - (1 - p)).max() <= 6 * sd(B * L * S)                    # every head
    assert np.abs(keep.mean(axis=3) - (1 - p)).max() <= 6 * sd(S)                                     # every query row
    # a key keeps its decision when the row grows, and batch 1 is not batch 0: the mask depends on (seed, b * H + h, query, key)
    assert np.array_equal(decoder._dropout_keep_host(11, 1, H, 5, 100, p), keep[:, :, :5, :100])
    two = decoder._dropout_keep_host(11, 2, H, 5, 100, p)
    assert np.array_equal(two[0], keep[0, :, :5, :100]) and not np.array_equal(two[0], two[1])
    assert decoder._dropout_keep_host(11, 1, 1, 4, 64, 0.0).all()
