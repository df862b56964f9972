"""Writes tests/golden/fused_routes.json: which kernel every convolution of the fused sparse encoder takes, per level, over the
switch-over points of the routing tables of bevfusion_amd/spconv/fused.py.  tests/test_fused_routes.py pins `_route_for` to it.

The file is a record of the commit BEFORE the routing moved into `_route_for`: this script only uses names that exist on both
sides (`_slab_variant_for`, `_variant_for`, `ops.slab_block_rows`, `ops.get_conv_output_size`, `_chain_modules`) and restates how
that commit's `_conv` / `_geometry_steps` combined them.  It needs the built library (host-only queries) and no GPU, and refuses
to run with any BEVAMD_SPCONV_* variable set.

    python tests/golden/make_fused_routes_golden.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(HERE, "fused_routes.json")
# (frames_hint, batch): no hint -> the batch size stands in for it; the hints sit on both sides of every threshold of the tables
# (_SLAB_SMALL_BATCH_BELOW 1.5 / 2.5, the historical 3.5 / 4, _variant_for's 5.5)
FRAMES = [(None, 1), (None, 2), (None, 8)] + [(h, 2) for h in (1.0, 1.4, 1.6, 2.4, 2.6, 4.0, 5.4, 5.6, 8.0)]


def encoders():
    """name -> encoder, on the CPU: the flagship (tests/test_gpu_keyorder.py) and the small one (tests/test_gpu_spconv_fused.py)."""
    from bevfusion_amd import synth
    from bevfusion_amd.sparse_encoder import SparseEncoder

    common = dict(order=["conv", "norm", "act"], encoder_paddings=[[0, 0, 1], [0, 0, 1], [0, 0, [1, 1, 0]], [0, 0]], block_type="basicblock")
    return {"flagship": SparseEncoder(5, list(synth.CL_CONFIG["sparse_shape"]), output_channels=128,
                                      encoder_channels=[[16, 16, 32], [32, 32, 64], [64, 64, 128], [128, 128]], **common),
            "small": SparseEncoder(5, [40, 40, 41], output_channels=32,
                                   encoder_channels=[[16, 16, 32], [32, 32, 64], [64, 64, 64], [64, 64]], **common)}


def cases():
    for name in ("flagship", "small"):
        for linear in (False, True):
            for allow_slab in (True, False):
                for hint, batch in FRAMES:
                    for profile in (False, True):
                        yield dict(encoder=name, linear=linear, allow_slab=allow_slab, frames_hint=hint, batch=batch, profile=profile)


def level_chain(enc, case):
    """[(conv, the Level it reads)] over empty CPU index tensors: level 1 as the caller describes it, every later level as a strided
    convolution leaves it (rank index, rows in linear order)."""
    from bevfusion_amd.spconv import fused, ops

    def level(shape, linear):
        lvl = fused.Level(torch.empty((0, 4), dtype=torch.int32), 0, None, case["batch"], shape, linear_order=linear,
                          allow_slab=case["allow_slab"])
        lvl.frames_hint = case["frames_hint"]
        return lvl

    cur, out = level(enc.sparse_shape, case["linear"]), []
    for m in fused._chain_modules(enc):
        out.append((m, cur))
        if not m.subm:
            cur = level(ops.get_conv_output_size(cur.shape, list(m.kernel_size), list(m.stride), list(m.padding), [1, 1, 1]), True)
            cur.index_kind = fused.INDEX_RANK
    return out


def parent_routes(enc, case):
    """[kernel, variant, block rows, int32 table wanted] per convolution, as the parent commit's `_conv` decided them."""
    from bevfusion_amd.spconv import fused, ops

    rows = []
    for m, lvl in level_chain(enc, case):
        cin, cout = m.in_channels, m.out_channels
        K = m.kernel_size[0] * m.kernel_size[1] * m.kernel_size[2]
        frames = float(lvl.batch) if lvl.frames_hint is None else lvl.frames_hint
        v = fused._slab_variant_for(m, lvl, cin, cout)
        if v is not None:
            rows.append(["slab", int(v), int(ops.slab_block_rows(cin, v)), bool(case["profile"])])
        else:
            rows.append(["gather", int(fused._variant_for(frames, K, cin, cout)), 0, True])
    return rows


def main():
    set_ = sorted(k for k in os.environ if k.startswith("BEVAMD_SPCONV_"))
    if set_:
        sys.exit(f"unset {', '.join(set_)} first: the golden records the default routes")
    from bevfusion_amd.spconv import fused

    encs = encoders()
    out = []
    for case in cases():
        fused.LAYER_PROFILE = [] if case["profile"] else None
        try:
            out.append(dict(case, layers=parent_routes(encs[case["encoder"]], case)))
        finally:
            fused.LAYER_PROFILE = None
    with open(GOLDEN, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in out) + "\n]\n")
    print(f"wrote {GOLDEN}: {len(out)} cases")


if __name__ == "__main__":
    main()
