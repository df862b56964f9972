"""The fused sparse encoder issues the same native calls as the commit before its routing, product cache and pass brackets were
gathered into one place each (spconv/fused.py, spconv/fused_train.py): same entry points, same order, same stream (main or
geometry), same kernel variant.  tests/golden/fused_call_trace.json was recorded at that commit on an MI355X by

    python tests/test_gpu_fused_call_trace.py --write

`_capi.load` is replaced by a proxy that logs every `bevamd_*` call: [name, "geom" | "main" | None, variant | None].  The middle
entry is None for a host-only query (sizes, capabilities: no stream argument, nothing is launched).  The launches are compared
entry by entry; the host-only queries are not kernels and a pass may make fewer of them than the recorded commit (a route that
carries its block size does not ask for it again), never more.

Passes (the small encoder and the inputs of test_fused_encoder_matches_module_path: grid (40, 40, 41), B = 2, 2 500 voxels per
sample): inference over rows in first-appearance order, in linear order, in linear order with the live-row figure forced to 8
frames (batched tilings, wave-pair 32-channel kernel), prepare_geometry + forward(geometry=), one fp16-autocast training step."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_call_trace.json")
B, SHAPE, PER_SAMPLE = 2, (40, 40, 41), 2500


class _Recorder:
    """Stands in for the library handle: forwards every attribute, logs the calls of the bevamd_* functions."""

    def __init__(self, lib, signatures, geom_handle):
        self._lib, self._signatures, self._geom, self.log = lib, signatures, geom_handle, None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("bevamd_"):
            return fn
        res, argtypes = self._signatures.get(name, (None, []))
        launches = res is ctypes.c_int and bool(argtypes) and argtypes[-1] is ctypes.c_void_p

        def call(*args):
            if self.log is not None:
                stream = None
                if launches:
                    handle = args[-1].value if isinstance(args[-1], ctypes.c_void_p) else args[-1]
                    stream = "geom" if (handle or 0) == self._geom else "main"
                self.log.append([name, stream, int(args[-2]) if "_conv_forward_" in name else None])
            return fn(*args)

        return call


def _inputs(dev):
    rng = np.random.default_rng(5)
    idx = []
    for b in range(B):
        lin = rng.choice(int(np.prod(SHAPE)), size=PER_SAMPLE, replace=False)
        idx.append(np.concatenate([np.full((len(lin), 1), b), np.stack(np.unravel_index(lin, SHAPE), 1)], 1))
    first = np.concatenate(idx).astype(np.int32)
    rng.shuffle(first, axis=0)
    c = first.astype(np.int64)
    linear = first[np.argsort(((c[:, 0] * SHAPE[0] + c[:, 1]) * SHAPE[1] + c[:, 2]) * SHAPE[2] + c[:, 3])]
    feats = rng.standard_normal((first.shape[0], 5)).astype(np.float32)
    return torch.from_numpy(feats).to(dev), torch.from_numpy(first).to(dev), torch.from_numpy(linear).to(dev)


def _encoder(dev, dtype):
    from test_gpu_spconv_fused import _small_encoder

    return _small_encoder(dev, dtype)


def record(dev):
    """{pass name: [[name, stream, variant], ...]} of the five passes."""
    from bevfusion_amd import _capi
    from bevfusion_amd.spconv import fused

    feats, first, linear = _inputs(dev)
    geom = fused.geometry_stream(dev)
    assert geom is not None, "the trace is of the two-stream schedule"
    rec = _Recorder(_capi.load(), dict(_capi._SIGNATURES, **_capi._EXT_SIGNATURES), geom.cuda_stream)
    traces = {}

    def traced(name, fn):
        rec.log = []
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            traces[name], rec.log = rec.log, None

    real_load = _capi.load
    _capi.load = lambda: rec
    try:
        with torch.no_grad():
            x16 = feats.half()
            # eager inference: the SECOND call of each encoder (the first one reads the status words back and is not the steady state)
            enc = _encoder(dev, torch.float16)
            enc(x16, first, B)
            traced("inference_first_order", lambda: enc(x16, first, B))
            enc = _encoder(dev, torch.float16)
            enc(x16, linear, B, coors_order="linear")
            traced("inference_linear_order", lambda: enc(x16, linear, B, coors_order="linear"))
            traced("prepared_geometry", lambda: enc(x16, linear, B, geometry=enc.prepare_geometry(linear, B, coors_order="linear")))
            assert enc.last_path == "fused", enc.last_path_reason
            enc = _encoder(dev, torch.float16)
            enc.__dict__["_bevamd_frames_hint"] = {B: 8.0}
            enc(x16, linear, B, coors_order="linear")
            traced("inference_linear_order_8_frames", lambda: enc(x16, linear, B, coors_order="linear"))
            assert enc.last_path == "fused", enc.last_path_reason
        enc = _encoder(dev, torch.float32).train()

        def step():
            with torch.autocast("cuda", dtype=torch.float16):
                out = enc(feats, linear, B, coors_order="linear")
            assert enc.last_path == "fused-train", enc.last_path_reason
            out.float().square().mean().backward()

        step()                                  # the first call checks the status words up front
        traced("training_step_fp16_autocast", step)
    finally:
        _capi.load = real_load
    return traces


@pytest.mark.gpu
def test_fused_passes_issue_the_recorded_native_calls(dev):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = record(dev)
    assert sorted(got) == sorted(want)
    for name in want:
        launches = [c for c in got[name] if c[1] is not None]
        recorded = [c for c in want[name] if c[1] is not None]
        print(f"{name}: {len(launches)} launches ({len(recorded)} recorded), {len(got[name]) - len(launches)} host-only queries "
              f"({len(want[name]) - len(recorded)} recorded)")
        for i, (a, b) in enumerate(zip(launches, recorded)):
            assert a == b, f"{name}: launch {i} is {a}, recorded {b}"
        assert len(launches) == len(recorded), name
        assert len(got[name]) - len(launches) <= len(want[name]) - len(recorded), f"{name}: more host-only queries than recorded"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--write"], __doc__
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    traces = record(torch.device("cuda:0"))
    with open(GOLDEN, "w") as fh:
        fh.write("{\n" + ",\n".join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in traces.items()) + "\n}\n")
    print({k: len(v) for k, v in traces.items()})
