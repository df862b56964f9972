"""Writes tests/golden/decoder_layer_ref.npz: recorded outputs of the REFERENCE's TransformerDecoderLayer on seeded inputs.

The reference's `mmdet3d/models/utils/transformer.py` is read and exec'd at run time on CPU torch with one thread; `mmcv` and
`mmcv.cnn`, which it imports for its `FFN` class only, are stubbed with placeholders for `ConvModule`, `build_conv_layer` and
`kaiming_init`.  Nothing of the reference's text is stored: only the SHA-256 of the seeded inputs and weights and the recorded
results.  Inputs and weights are NOT stored: `case_inputs` / `layer_weights` regenerate them with numpy alone (the tests import this
file for them and check the stored digest).

The case: B = 2, Pq = 17, Pk = 53, d_model = 128, 8 heads, ffn 256, learned position embeddings of 2-d positions in [0, 180) on both
sides (the TransFusion configuration), xavier-uniform matrices, non-trivial BatchNorm running statistics and LayerNorm affine.
Recorded for the full layer and for cross_only=True: the state-dict names and shapes, the float64 eval-mode output (a deep copy
`.double()`), the fp32 output, and — for the cross-attention — the float64 inputs of `multi_head_attention_forward` and its output.

    python tests/golden/make_decoder_layer_golden.py
"""
import copy
import functools
import hashlib
import os
import sys
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "decoder_layer_ref.npz")
REF = "/root/reference/mmdet3d"

B, PQ, PK, D_MODEL, HEADS, FFN_DIM, POS_DIM = 2, 17, 53, 128, 8, 256, 2
INPUT_SEED = 1409


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def layer_shapes(cross_only=False, d_model=D_MODEL, ffn=FFN_DIM, pos_dim=POS_DIM):
    """name -> shape of the layer's state dict, in the reference's order (main() asserts it equals the reference's)."""
    shapes = {}

    def attn(prefix):
        shapes[prefix + ".in_proj_weight"] = (3 * d_model, d_model)
        shapes[prefix + ".in_proj_bias"] = (3 * d_model,)
        shapes[prefix + ".out_proj.weight"] = (d_model, d_model)
        shapes[prefix + ".out_proj.bias"] = (d_model,)

    def posembed(prefix):
        head = prefix + ".position_embedding_head."
        shapes[head + "0.weight"], shapes[head + "0.bias"] = (d_model, pos_dim, 1), (d_model,)
        for name in ("weight", "bias", "running_mean", "running_var"):
            shapes[head + "1." + name] = (d_model,)
        shapes[head + "1.num_batches_tracked"] = ()
        shapes[head + "3.weight"], shapes[head + "3.bias"] = (d_model, d_model, 1), (d_model,)

    if not cross_only:
        attn("self_attn")
    attn("multihead_attn")
    shapes["linear1.weight"], shapes["linear1.bias"] = (ffn, d_model), (ffn,)
    shapes["linear2.weight"], shapes["linear2.bias"] = (d_model, ffn), (d_model,)
    for i in (1, 2, 3):
        shapes[f"norm{i}.weight"], shapes[f"norm{i}.bias"] = (d_model,), (d_model,)
    posembed("self_posembed")
    posembed("cross_posembed")
    return shapes


@functools.lru_cache(maxsize=None)
def _weights(cross_only):
    out = {}
    for name, shape in layer_shapes(cross_only).items():
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        if name.endswith("num_batches_tracked"):
            value = np.array(7, np.int64)
        elif len(shape) >= 2:                                         # xavier uniform over (fan_out, fan_in, receptive field)
            field = int(np.prod(shape[2:]))
            bound = np.sqrt(6.0 / ((shape[0] + shape[1]) * field))
            value = rng.uniform(-bound, bound, shape).astype(np.float32)
        elif name.endswith("running_mean"):
            value = rng.uniform(-20.0, 20.0, shape).astype(np.float32)  # positions reach 180: the first conv's outputs are tens
        elif name.endswith("running_var"):
            value = rng.uniform(200.0, 800.0, shape).astype(np.float32)
        elif name.endswith(".weight"):                                # BatchNorm / LayerNorm scale
            value = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        else:                                                         # biases, BatchNorm / LayerNorm shift
            value = rng.uniform(-0.2, 0.2, shape).astype(np.float32)
        out[name] = value
    return out


def layer_weights(cross_only=False):
    """name -> fp32 array (int64 for num_batches_tracked), from seeds."""
    return dict(_weights(bool(cross_only)))


@functools.lru_cache(maxsize=None)
def case_inputs():
    """(query [B, C, Pq], key [B, C, Pk], query_pos [B, Pq, 2], key_pos [B, Pk, 2]) fp32."""
    rng = np.random.default_rng(INPUT_SEED)
    query = rng.standard_normal((B, D_MODEL, PQ)).astype(np.float32)
    key = rng.standard_normal((B, D_MODEL, PK)).astype(np.float32)
    query_pos = rng.uniform(0, 180, (B, PQ, POS_DIM)).astype(np.float32)
    key_pos = rng.uniform(0, 180, (B, PK, POS_DIM)).astype(np.float32)
    return query, key, query_pos, key_pos


def digest(cross_only=False):
    w = layer_weights(cross_only)
    return sha(*case_inputs(), *[w[name] for name in w])


def load_reference():
    import torch

    torch.set_num_threads(1)
    placeholders = dict(ConvModule=object, build_conv_layer=lambda *a, **k: None, kaiming_init=lambda *a, **k: None)
    saved = {name: sys.modules.get(name) for name in ("mmcv", "mmcv.cnn")}
    mmcv, cnn = types.ModuleType("mmcv"), types.ModuleType("mmcv.cnn")
    cnn.__dict__.update(placeholders)
    mmcv.cnn = cnn
    sys.modules["mmcv"], sys.modules["mmcv.cnn"] = mmcv, cnn
    try:
        path = os.path.join(REF, "models/utils/transformer.py")
        ns = {"__name__": "reference_transformer"}
        exec(compile(open(path).read(), path, "exec"), ns)
    finally:
        for name, module in saved.items():
            if module is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = module
    return ns


def record(ns, cross_only, out):
    import torch

    tag = "cross_only" if cross_only else "full"
    layer = ns["TransformerDecoderLayer"](D_MODEL, HEADS, FFN_DIM, dropout=0.1, activation="relu",
                                          self_posembed=ns["PositionEmbeddingLearned"](POS_DIM, D_MODEL),
                                          cross_posembed=ns["PositionEmbeddingLearned"](POS_DIM, D_MODEL), cross_only=cross_only)
    state = layer.state_dict()
    assert {k: tuple(v.shape) for k, v in state.items()} == layer_shapes(cross_only) and list(state) == list(layer_shapes(cross_only))
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in layer_weights(cross_only).items()}, strict=True)
    layer.eval()
    inputs = [torch.from_numpy(a) for a in case_inputs()]
    with torch.no_grad():
        out32 = layer(*inputs)
        layer64 = copy.deepcopy(layer).double()
        seen = {}

        def hook(module, args, kwargs):
            seen.update(query=kwargs["query"], key=kwargs["key"], value=kwargs["value"])

        handle = layer64.multihead_attn.register_forward_pre_hook(hook, with_kwargs=True)
        out64 = layer64(*[a.double() for a in inputs])
        handle.remove()
        attn = layer64.multihead_attn
        assert torch.equal(seen["key"], seen["value"])
        attn64 = ns["multi_head_attention_forward"](seen["query"], seen["key"], seen["value"], D_MODEL, HEADS, attn.in_proj_weight,
                                                    attn.in_proj_bias, None, None, False, 0.0, attn.out_proj.weight, attn.out_proj.bias,
                                                    training=False, need_weights=False)[0]
    out[f"{tag}.names"] = np.array(list(state))
    out[f"{tag}.shapes"] = np.array([",".join(str(d) for d in v.shape) for v in state.values()])
    out[f"{tag}.out64"] = out64.numpy()
    out[f"{tag}.out32"] = out32.numpy()
    out[f"{tag}.attn_query64"] = seen["query"].numpy()
    out[f"{tag}.attn_key64"] = seen["key"].numpy()
    out[f"{tag}.attn_out64"] = attn64.numpy()
    out[f"{tag}.inputs_sha256"] = np.array(digest(cross_only))
    err = float((out32.double() - out64).abs().max())
    print(f"  {tag}: {len(state)} state entries, |out| max {float(out64.abs().max()):.3f}, fp32 against float64 {err:.3e}")


def main():
    ns = load_reference()
    out = {}
    record(ns, False, out)
    record(ns, True, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
