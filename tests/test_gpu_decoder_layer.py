"""GPU: the fused decoder attention and the decoder layer against the float64 host mirrors.

Bars are measured, not chosen: on the same GPU the reference's formulation (`bmm`, `softmax`, `bmm` as fp32 torch ops,
`decoder._attention_torch`) runs on the same inputs, and the kernel's largest absolute error against float64 must not exceed TWICE
that formulation's (the factor covers another summation order over up to 32 400 keys and the split merge; both sides round in fp32).
Where the torch error is below 1e-6 the bar is 2e-6.  The same bar holds for out, lse, the gradients and the layer.  Both errors of
every case are recorded through conftest.record_parity: `<case>` carries the kernel's error, `<case>_torch` the torch formulation's,
each next to the enforced bar."""
import functools
import importlib.util
import os
import zlib
from unittest import mock

import numpy as np
import pytest
import torch

from bevfusion_amd import decoder
from conftest import record_parity

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_decoder_layer_golden", os.path.join(HERE, "golden", "make_decoder_layer_golden.py"))
MAKER = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MAKER)
GOLDEN = np.load(os.path.join(HERE, "golden", "decoder_layer_ref.npz"))

K0 = decoder.SPLIT_KEYS_MIN
ONE_SPLIT_PLUS_1 = (1, 8, 200, K0 + 1)                     # two splits: K0 keys and 1 key
THREE_RAGGED = (1, 8, 200, 2 * K0 + 37)                    # three splits, the last one ragged
BWD_THREE_RAGGED = (1, 8, 200, 2 * decoder.BACKWARD_BLOCK_KEYS + 37)      # three backward key blocks, the last one ragged
FLAGSHIP = (1, 8, 200, 32400)
# 128 (sample, head) pairs: forward splits of 192 keys = three 64-key steps, so a maximum met in a split's second step rescales what
# the first step summed; backward key blocks of two 256-key chunks, the last block's second chunk wholly past S
MID = (8, 16, 17, 16 * decoder.BACKWARD_BLOCK_KEYS + 37)


def _bar(err_torch):
    return max(2.0 * float(err_torch), 2e-6)


def _record(name, err, err_torch, bar):
    record_parity(name, err, bar)
    record_parity(name + "_torch", err_torch, bar)


def _err(got, truth):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else got
    assert np.isfinite(got).all()
    return float(np.abs(got - truth).max())


@functools.lru_cache(maxsize=None)
def _inputs(shape, kind):
    """fp32 (q, k, v) with structure.  noise: unit normal.  spike / spike_last: row i of every head carries 16 on coordinate
    1 + i % 15 and key j_c carries 24 on coordinate c, so row i's logit at its key is 96 and every other one is below 36: the running
    maximum jumps mid-stream (spike_last: all 15 keys in the last 37 keys, the ragged split; spike_mid: key j_c in the second 64-key
    step of forward split c + 1, so the in-split rescale runs on a finite earlier maximum).  big: logits of standard deviation 20,
    extremes beyond +-80.  uniform: sample 0's keys are all equal, so its weights are uniform and out is the mean of v."""
    B, H, L, S = shape
    rng = np.random.default_rng(zlib.crc32(_name(shape, kind).encode()))
    q = rng.standard_normal((B, L, H, 16)).astype(np.float32)
    k = rng.standard_normal((B, S, H, 16)).astype(np.float32)
    v = rng.standard_normal((B, S, H, 16)).astype(np.float32)
    if kind in ("spike", "spike_last", "spike_mid"):
        assert S >= 53
        if kind == "spike_mid":
            split_keys = decoder.attention_plan(*shape)[1]
            assert split_keys >= 2 * K0 and 15 * split_keys + K0 + 15 <= S
            keys = np.array([(c + 1) * split_keys + K0 + c for c in range(15)])
        else:
            where = np.arange(S - 37, S) if kind == "spike_last" else np.arange(S // 3, S)
            keys = rng.choice(where, 15, replace=False)
        for c in range(15):
            k[:, keys[c], :, 1 + c] = 24.0
        for i in range(L):
            q[:, i, :, 1 + i % 15] = 16.0
    elif kind == "big":
        q *= 4.5
        k *= 4.5
    elif kind == "uniform":
        k[0] = k[0, :1]
    elif kind != "noise":
        raise ValueError(kind)
    return tuple(t.reshape(t.shape[0], t.shape[1], H * 16) for t in (q, k, v))


@functools.lru_cache(maxsize=None)
def _truth(shape, kind):
    q, k, v = _inputs(shape, kind)
    return decoder._attention_host(q, k, v, return_lse=True)


FORWARD_CASES = [((1, 1, 1, 1), "noise"), ((2, 8, 17, 53), "noise"), ((1, 8, 16, 16), "noise"), ((3, 2, 15, 17), "noise"),
                 ((2, 8, 17, 53), "spike"), ((2, 8, 17, 53), "big"), ((2, 8, 17, 53), "uniform"),
                 (ONE_SPLIT_PLUS_1, "noise"), (ONE_SPLIT_PLUS_1, "big"), (THREE_RAGGED, "noise"), (THREE_RAGGED, "spike"),
                 (THREE_RAGGED, "spike_last"), (THREE_RAGGED, "big"), (THREE_RAGGED, "uniform"),
                 (MID, "noise"), (MID, "spike_mid"), (FLAGSHIP, "noise"), (FLAGSHIP, "spike_last")]


def _name(shape, kind):
    return "x".join(str(s) for s in shape) + "/" + kind


def test_shapes_from_the_kernel_constants_split_as_meant():
    assert decoder.attention_plan(*ONE_SPLIT_PLUS_1)[:2] == (2, K0)
    assert decoder.attention_plan(*THREE_RAGGED)[:2] == (3, K0)
    assert decoder.attention_plan(*BWD_THREE_RAGGED)[2:] == (3, decoder.BACKWARD_BLOCK_KEYS)
    assert decoder.attention_plan(*FLAGSHIP)[0] > 1
    splits, split_keys, blocks, block_keys = decoder.attention_plan(*MID)
    assert split_keys == 3 * K0 and splits > 15                              # three steps per split
    assert block_keys == 2 * decoder.BACKWARD_BLOCK_KEYS                      # two chunks per backward key block ...
    assert (blocks * 2 - 1) * decoder.BACKWARD_BLOCK_KEYS >= MID[3]           # ... and the last block's second chunk holds no key


@pytest.mark.parametrize("shape,kind", FORWARD_CASES, ids=[_name(*c) for c in FORWARD_CASES])
def test_forward_fp32(shape, kind, dev):
    q, k, v = (torch.from_numpy(t).to(dev) for t in _inputs(shape, kind))
    want, want_lse = _truth(shape, kind)
    out, lse = decoder.fused_attention(q, k, v, return_lse=True)
    assert out.dtype == torch.float32 and out.shape == q.shape and tuple(lse.shape) == want_lse.shape
    B, L, E = q.shape
    H = E // 16
    qh = (q * 0.25).reshape(B, L, H, 16).permute(0, 2, 1, 3)
    kh = k.reshape(B, -1, H, 16).permute(0, 2, 1, 3)
    e_torch, e_torch_lse = _err(decoder._attention_torch(q, k, v), want), _err(torch.logsumexp(qh @ kh.transpose(2, 3), dim=-1), want_lse)
    e, e_lse = _err(out, want), _err(lse, want_lse)
    bar, bar_lse = _bar(e_torch), _bar(e_torch_lse)
    print(f"{_name(shape, kind)}: out {e:.3e} (torch {e_torch:.3e}, bar {bar:.3e}); lse {e_lse:.3e} (torch {e_torch_lse:.3e}, bar {bar_lse:.3e})")
    _record(f"decoder_attention/forward/{_name(shape, kind)}/out", e, e_torch, bar)
    _record(f"decoder_attention/forward/{_name(shape, kind)}/lse", e_lse, e_torch_lse, bar_lse)
    if kind.startswith("spike"):
        assert float(np.sort(want_lse.reshape(-1))[0]) > 90.0                  # the spike carries every row
    if kind == "uniform":
        mean = _inputs(shape, kind)[2][0].astype(np.float64).mean(0)
        assert np.abs(want[0] - mean).max() < 1e-12
    assert e <= bar and e_lse <= bar_lse
    assert torch.equal(decoder.fused_attention(q, k, v), out)                   # the plain call returns the same tensor contents


FP16_CASES = [((2, 8, 17, 53), "noise"), (THREE_RAGGED, "spike_last"), (FLAGSHIP, "noise")]


@pytest.mark.parametrize("shape,kind", FP16_CASES, ids=[_name(*c) for c in FP16_CASES])
def test_forward_fp16(shape, kind, dev):
    """fp16 inputs, fp32 softmax and sums, fp16 out: against float64 on the fp16-rounded inputs; the bar is twice the error of the
    same torch formulation run in fp16 on the GPU."""
    scale = 0.25 if kind.startswith("spike") else 1.0                           # the planted 16 x 24 stay inside fp16's logit range
    q, k, v = (torch.from_numpy(t).to(dev).half() for t in _inputs(shape, kind))
    q = q * scale
    want = decoder._attention_host(q.cpu().float().numpy(), k.cpu().float().numpy(), v.cpu().float().numpy())
    out = decoder.fused_attention(q, k, v)
    assert out.dtype == torch.float16
    e, e_torch = _err(out, want), _err(decoder._attention_torch(q, k, v), want)
    bar = _bar(e_torch)
    print(f"fp16 {_name(shape, kind)}: out {e:.3e} (torch fp16 {e_torch:.3e}, bar {bar:.3e})")
    _record(f"decoder_attention/forward_fp16/{_name(shape, kind)}/out", e, e_torch, bar)
    assert e <= bar
    # with a gradient needed the inputs are upcast: the fp32 kernels serve forward and backward
    qg = q.clone().requires_grad_()
    og = decoder.fused_attention(qg, k, v)
    og.float().sum().backward()
    assert og.dtype == torch.float16 and qg.grad.dtype == torch.float16 and _err(og, want) <= bar


def _grads(fn, q, k, v, dout):
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = fn(q, k, v)
    out.backward(dout)
    return out.detach(), [q.grad, k.grad, v.grad]


BACKWARD_CASES = [((2, 8, 17, 53), "noise"), (BWD_THREE_RAGGED, "noise"), (BWD_THREE_RAGGED, "spike"), (BWD_THREE_RAGGED, "spike_last"),
                  ((3, 2, 15, 17), "noise"), (MID, "noise"), (MID, "spike_mid")]


def _check_backward(shape, kind, dev, p=0.0, seed=0):
    arrays = _inputs(shape, kind)
    B, H, L, S = shape
    rng = np.random.default_rng(5)
    dout = rng.standard_normal(arrays[0].shape).astype(np.float32)
    keep = torch.from_numpy(decoder._dropout_keep_host(seed, B, H, L, S, p)) if p > 0 else None
    host = [torch.from_numpy(t).double() for t in arrays]
    want_out, want = _grads(lambda q, k, v: decoder._attention_torch(q, k, v, keep, p), *host, torch.from_numpy(dout).double())
    gpu = [torch.from_numpy(t).to(dev) for t in arrays]
    keep_dev = keep.to(dev) if keep is not None else None
    _, ref = _grads(lambda q, k, v: decoder._attention_torch(q, k, v, keep_dev, p), *gpu, torch.from_numpy(dout).to(dev))
    out, got = _grads(lambda q, k, v: decoder.fused_attention(q, k, v, dropout_p=p, seed=seed), *gpu, torch.from_numpy(dout).to(dev))
    tag = f"{_name(shape, kind)}" + (f"/p{p}" if p else "")
    worst = []
    for name, g, r, w in zip(("dq", "dk", "dv"), got, ref, want):
        w = w.numpy()
        e, e_torch = _err(g, w), _err(r, w)
        bar = _bar(e_torch)
        print(f"backward {tag}: {name} {e:.3e} (torch {e_torch:.3e}, bar {bar:.3e}, |{name}| max {np.abs(w).max():.3e})")
        _record(f"decoder_attention/backward/{tag}/{name}", e, e_torch, bar)
        worst.append((name, e, bar))
    return out, got, want_out.numpy(), worst


@pytest.mark.parametrize("shape,kind", BACKWARD_CASES, ids=[_name(*c) for c in BACKWARD_CASES])
def test_backward_fp32(shape, kind, dev):
    _, _, _, worst = _check_backward(shape, kind, dev)
    assert all(e <= bar for _, e, bar in worst), worst


DROPOUT_CASES = [(1, 8, 17, K0), (1, 8, 17, K0 + 1), BWD_THREE_RAGGED]


@pytest.mark.parametrize("shape", DROPOUT_CASES, ids=["x".join(str(s) for s in c) for c in DROPOUT_CASES])
def test_dropout_equals_the_host_mask(shape, dev):
    """p = 0.1 with a fixed seed: forward and backward equal the host formula under `_dropout_keep_host`'s mask.  K0 and K0 + 1 keys
    straddle a split boundary (one split, two splits) under one mask mirror: the mask does not depend on the split count."""
    p, seed = 0.1, 20261019
    out, got, want_out, worst = _check_backward(shape, "noise", dev, p=p, seed=seed)
    arrays = _inputs(shape, "noise")
    gpu = [torch.from_numpy(t).to(dev) for t in arrays]
    keep = torch.from_numpy(decoder._dropout_keep_host(seed, *shape, p)).to(dev)
    e, e_torch = _err(out, want_out), _err(decoder._attention_torch(*gpu, keep, p), want_out)
    bar = _bar(e_torch)
    _record(f"decoder_attention/dropout/{'x'.join(str(s) for s in shape)}/out", e, e_torch, bar)
    print(f"dropout {shape}: out {e:.3e} (torch {e_torch:.3e}, bar {bar:.3e})")
    assert e <= bar and all(e <= bar for _, e, bar in worst), worst
    again = decoder.fused_attention(*gpu, dropout_p=p, seed=seed)
    assert torch.equal(again, out)
    other = decoder.fused_attention(*gpu, dropout_p=p, seed=seed + 1)
    assert not torch.equal(other, out)
    assert not torch.equal(decoder.fused_attention(*gpu), out)                   # and p = 0 is another result


def test_dropout_seed_comes_from_the_host_generator(dev):
    q, k, v = (torch.from_numpy(t).to(dev) for t in _inputs((2, 8, 17, 53), "noise"))
    torch.manual_seed(7)
    a = decoder.fused_attention(q, k, v, dropout_p=0.1)
    b = decoder.fused_attention(q, k, v, dropout_p=0.1)
    torch.manual_seed(7)
    assert torch.equal(decoder.fused_attention(q, k, v, dropout_p=0.1), a) and not torch.equal(a, b)
    attn = decoder.MultiheadAttention(128, 8, dropout=0.1).to(dev)
    x, mem = q.transpose(0, 1), k.transpose(0, 1)
    torch.manual_seed(9)
    first = attn(x, mem, mem)[0]
    torch.manual_seed(9)
    assert torch.equal(attn(x, mem, mem)[0], first)
    assert not torch.equal(attn.eval()(x, mem, mem)[0], first)                  # eval mode drops nothing


@pytest.mark.parametrize("shape", [BWD_THREE_RAGGED, FLAGSHIP], ids=["three_blocks", "flagship"])
def test_forward_and_backward_are_bit_reproducible(shape, dev):
    arrays = _inputs(shape, "noise")
    gpu = [torch.from_numpy(t).to(dev) for t in arrays]
    dout = torch.from_numpy(np.random.default_rng(3).standard_normal(arrays[0].shape).astype(np.float32)).to(dev)
    first = _grads(decoder.fused_attention, *gpu, dout)
    second = _grads(decoder.fused_attention, *gpu, dout)
    assert torch.equal(first[0], second[0])
    assert all(torch.equal(a, b) for a, b in zip(first[1], second[1]))


def test_views_off_the_16_byte_grid_are_served(dev):
    """A contiguous view whose storage offset is not a multiple of 16 bytes (the kernels load 16 bytes at a time) is copied, not
    refused: forward and backward equal the aligned call bit for bit."""
    arrays = _inputs((2, 8, 17, 53), "noise")
    aligned = [torch.from_numpy(t).to(dev) for t in arrays]
    dout = torch.from_numpy(np.random.default_rng(4).standard_normal(arrays[0].shape).astype(np.float32)).to(dev)

    def shifted(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
        view = flat[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view

    want = _grads(decoder.fused_attention, *aligned, dout)
    assert torch.equal(decoder.fused_attention(*[shifted(t) for t in aligned]), want[0])
    q, k, v = (shifted(t).requires_grad_() for t in aligned)
    out = decoder.fused_attention(q, k, v)
    out.backward(shifted(dout))
    assert torch.equal(out.detach(), want[0]) and all(torch.equal(a.grad, b) for a, b in zip((q, k, v), want[1]))


# ---- the layer -------------------------------------------------------------------------------------------------------------------
def _posembed():
    return decoder.PositionEmbeddingLearned(MAKER.POS_DIM, MAKER.D_MODEL)


def _layer(dev, cross_only=False, dropout=0.1):
    layer = decoder.TransformerDecoderLayer(MAKER.D_MODEL, MAKER.HEADS, MAKER.FFN_DIM, dropout=dropout, self_posembed=_posembed(),
                                            cross_posembed=_posembed(), cross_only=cross_only)
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in MAKER.layer_weights(cross_only).items()}, strict=True)
    return layer.to(dev)


def _torch_formulation():
    """The layer's attention replaced by the reference's formulation as torch ops: what the bars are measured with."""
    return mock.patch.object(decoder, "fused_attention", lambda q, k, v, dropout_p=0.0, seed=None: decoder._attention_torch(q, k, v))


@pytest.mark.parametrize("cross_only", [False, True], ids=["full", "cross_only"])
def test_layer_against_the_reference_golden(cross_only, dev):
    """eval mode, the golden's weights: within twice the recorded error of the reference's own fp32 output against its float64
    output (both in the golden)."""
    tag = "cross_only" if cross_only else "full"
    want = GOLDEN[f"{tag}.out64"]
    bar = 2.0 * float(np.abs(GOLDEN[f"{tag}.out32"].astype(np.float64) - want).max())
    layer = _layer(dev, cross_only).eval()
    inputs = [torch.from_numpy(a).to(dev) for a in MAKER.case_inputs()]
    with torch.no_grad():
        out = layer(*inputs)
        with _torch_formulation():
            e_torch = _err(layer(*inputs), want)
    e = _err(out, want)
    print(f"layer {tag}: {e:.3e} (torch ops on this GPU {e_torch:.3e}, bar {bar:.3e}: twice the reference's fp32 error)")
    _record(f"decoder_layer/golden/{tag}", e, e_torch, bar)
    assert tuple(out.shape) == want.shape and e <= bar


def test_layer_at_the_configuration_shape(dev):
    """B = 1, 200 queries, 32 400 BEV keys against `_layer_host`; the bar is twice the error of the same layer with the attention as
    fp32 torch ops on this GPU."""
    rng = np.random.default_rng(41)
    query = rng.standard_normal((1, MAKER.D_MODEL, 200)).astype(np.float32)
    key = rng.standard_normal((1, MAKER.D_MODEL, 32400)).astype(np.float32)
    query_pos = rng.uniform(0, 180, (1, 200, 2)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(180, dtype=np.float32) + 0.5, np.arange(180, dtype=np.float32) + 0.5, indexing="ij")
    key_pos = np.stack([xs, ys], -1).reshape(1, 32400, 2)
    want = decoder._layer_host(MAKER.layer_weights(), query, key, query_pos, key_pos, nhead=MAKER.HEADS).numpy()
    layer = _layer(dev).eval()
    inputs = [torch.from_numpy(a).to(dev) for a in (query, key, query_pos, key_pos)]
    with torch.no_grad():
        out = layer(*inputs)
        with _torch_formulation():
            e_torch = _err(layer(*inputs), want)
    e, bar = _err(out, want), _bar(e_torch)
    print(f"layer 200 x 32400: {e:.3e} (torch {e_torch:.3e}, bar {bar:.3e})")
    _record("decoder_layer/200x32400", e, e_torch, bar)
    assert e <= bar


def test_layer_gradients(dev):
    """Train mode with all dropouts 0 (BatchNorm on batch statistics), a scalar loss: every parameter gradient and both input gradients
    against `_layer_host`'s in float64; bars from the same layer with the attention as fp32 torch ops on this GPU."""
    arrays = MAKER.case_inputs()
    weight = np.random.default_rng(8).standard_normal((MAKER.B, MAKER.D_MODEL, MAKER.PQ))
    state = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_() for k, v in MAKER.layer_weights().items()
             if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    host_in = [torch.from_numpy(a).double() for a in arrays]
    host_in[0].requires_grad_(), host_in[1].requires_grad_()
    loss = (decoder._layer_host(state, *host_in, nhead=MAKER.HEADS, training=True) * torch.from_numpy(weight)).sum()
    loss.backward()
    want = {k: v.grad.numpy() for k, v in state.items()}
    want["input.query"], want["input.key"] = host_in[0].grad.numpy(), host_in[1].grad.numpy()

    def device_grads(patched):
        layer = _layer(dev, dropout=0.0).train()
        inputs = [torch.from_numpy(a).to(dev) for a in arrays]
        inputs[0].requires_grad_(), inputs[1].requires_grad_()
        w = torch.from_numpy(weight).float().to(dev)
        if patched:
            with _torch_formulation():
                (layer(*inputs) * w).sum().backward()
        else:
            (layer(*inputs) * w).sum().backward()
        grads = {k: p.grad for k, p in layer.named_parameters()}
        grads["input.query"], grads["input.key"] = inputs[0].grad, inputs[1].grad
        return grads

    got, ref = device_grads(False), device_grads(True)
    assert set(got) == set(want) and len(want) == 32
    failed = []
    for name in sorted(want):
        e, e_torch = _err(got[name], want[name]), _err(ref[name], want[name])
        bar = _bar(e_torch)
        print(f"layer grad {name}: {e:.3e} (torch {e_torch:.3e}, bar {bar:.3e}, max {np.abs(want[name]).max():.3e})")
        _record(f"decoder_layer/grad/{name}", e, e_torch, bar)
        if e > bar:
            failed.append((name, e, bar))
    assert not failed, failed


def test_no_host_sync_and_graph_replay(dev):
    """Forward only, eval mode, no gradient: a warmed `fused_attention` call and a warmed layer call under sync debug mode "error";
    the layer captured once after a side-stream warm-up and replayed over three fresh contents, each replay bit-equal to eager."""
    layer = _layer(dev).eval()
    rng = np.random.default_rng(12)

    def fresh():
        return [torch.from_numpy(rng.standard_normal((2, MAKER.D_MODEL, 17)).astype(np.float32)).to(dev),
                torch.from_numpy(rng.standard_normal((2, MAKER.D_MODEL, 3 * K0 + 5)).astype(np.float32)).to(dev),
                torch.from_numpy(rng.uniform(0, 180, (2, 17, 2)).astype(np.float32)).to(dev),
                torch.from_numpy(rng.uniform(0, 180, (2, 3 * K0 + 5, 2)).astype(np.float32)).to(dev)]

    static = fresh()
    q, k, v = (torch.from_numpy(t).to(dev) for t in _inputs(THREE_RAGGED, "noise"))
    with torch.no_grad():
        warm_attention, warm_layer = decoder.fused_attention(q, k, v), layer(*static)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again_attention, again_layer = decoder.fused_attention(q, k, v), layer(*static)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(again_attention, warm_attention) and torch.equal(again_layer, warm_layer)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            layer(*static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                       # a capture admits no sync and no read-back
            out = layer(*static)
        for _ in range(3):
            contents = fresh()
            for dst, src in zip(static, contents):
                dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, layer(*contents))
