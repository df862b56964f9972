"""`fused._route_for` — the one place that decides which kernel, variant, block size and rulebook product a convolution of the
fused sparse encoder takes — reproduces tests/golden/fused_routes.json, recorded from the commit before that function existed
(tests/golden/make_fused_routes_golden.py): both encoders, level 1 in either row order, slab kernels allowed or not, frame counts
on both sides of every threshold of the tables, profiled or not.  `_slab_variant_for` / `_variant_for` keep their results too.
Needs the library's host-only queries, no GPU."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_fused_routes_golden", os.path.join(HERE, "golden", "make_fused_routes_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def maker():
    return _load_maker()


@pytest.fixture(scope="module")
def golden(maker):
    with open(maker.GOLDEN) as fh:
        return json.load(fh)


def test_golden_covers_every_case(maker, golden):
    assert [{k: v for k, v in c.items() if k != "layers"} for c in golden] == list(maker.cases())


def test_route_for_reproduces_the_recorded_routes(maker, golden, monkeypatch):
    from bevfusion_amd.spconv import fused, ops

    assert fused._SLAB and not fused._SLAB_OVERRIDES, "BEVAMD_SPCONV_SLAB / _SLAB_VARIANTS are set: the golden records the defaults"
    encs = maker.encoders()
    for case in golden:
        monkeypatch.setattr(fused, "LAYER_PROFILE", [] if case["profile"] else None)
        chain = maker.level_chain(encs[case["encoder"]], case)
        assert len(chain) == len(case["layers"])
        for i, ((conv, lvl), (kernel, variant, rows, want_nbr)) in enumerate(zip(chain, case["layers"])):
            where = ({k: v for k, v in case.items() if k != "layers"}, i)
            route = fused._route_for(conv, lvl)
            assert tuple(route) == (kernel, variant, rows, want_nbr), where
            assert (route.kernel, route.variant, route.block_rows, route.want_nbr) == tuple(route)
            cin, cout = conv.in_channels, conv.out_channels
            slab = fused._slab_variant_for(conv, lvl, cin, cout)
            if kernel == "slab":
                assert slab == variant and ops.slab_block_rows(cin, slab) == rows, where
            else:
                K = conv.kernel_size[0] * conv.kernel_size[1] * conv.kernel_size[2]
                frames = float(lvl.batch) if lvl.frames_hint is None else lvl.frames_hint
                assert slab is None and fused._variant_for(frames, K, cin, cout) == variant, where
