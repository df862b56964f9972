"""GPU: `bevamd_depth_inputs_batch{,_zero_ws}` (csrc/vtransform.hip) and `BaseDepthTransform` on device tensors with every depth-input
option of the reference (base.py:266-329), against tests/golden/depth_inputs_ref.npz (the reference's own forward on CPU torch) and
the numpy restatement of tests/test_depth_inputs.py.  Every comparison is on the raw bits: no tolerance anywhere.

The module's default device path inverts the LiDAR augmentation with `bevamd_mat3_inverse_with_column` (fp64 adjugate, within 1 ulp of
LAPACK's result but not its bits), so the module is tied to the fixture twice: `lapack_inverse=True` with `torch.inverse` answering
what the reference's own calls returned (recorded in the fixture) must give the fixture's bits, and the default path must give the
bits of the C-ABI entry on the device-computed inverse."""
import ctypes

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi, vtransforms
from test_depth_inputs import (CASES, CFG, MODES, N_CAM, clouds_of, dense_reference, gold, make_cloud, make_module, restate,  # noqa: F401
                               run_forward)

pytestmark = pytest.mark.gpu
IDS = [f"{c}-{m[0]}" for c, m in CASES]
IH, IW = CFG["image_size"]


def g(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def mode_args(mode, n_bins=59):
    _, depth_input, expand, feats = mode
    return (1 if depth_input == "one-hot" else 0, n_bins if depth_input == "one-hot" else 0, int(expand), int(feats))


def depth_inputs(dev, pts, inv, trans, l2i, ia, ih, iw, margs, ws=None, zero_ws=False):
    """One call of the C-ABI entry on device tensors -> depth [B, ncam, Cd, ih, iw]."""
    lib = _capi.load()
    B, n_cam, F = len(pts), l2i.shape[1], pts[0].shape[1]
    cd = lib.bevamd_depth_inputs_channels(margs[0], margs[1], F, margs[3])
    assert cd == (margs[1] if margs[0] else 1) + (F if margs[3] else 0)
    depth = torch.empty((B, n_cam, cd, ih, iw), dtype=torch.float32, device=dev)
    ptrs = (ctypes.c_void_p * B)(*[p.data_ptr() if p.shape[0] else None for p in pts])
    counts = (ctypes.c_int * B)(*[int(p.shape[0]) for p in pts])
    wsb = lib.bevamd_depth_raster_workspace_bytes(n_cam, ih, iw) * B
    if ws is None:
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    fn = lib.bevamd_depth_inputs_batch_zero_ws if zero_ws else lib.bevamd_depth_inputs_batch
    _capi.check(fn(ptrs, counts, B, F, _capi.ptr(inv), _capi.ptr(trans), 3, _capi.ptr(l2i), _capi.ptr(ia), n_cam, ih, iw, *margs,
                   _capi.ptr(depth), _capi.ptr(ws), wsb, _capi.stream_ptr(dev)), "depth_inputs_batch")
    return depth


def device_inverse(dev, la):
    lib = _capi.load()
    B = la.shape[0]
    inv = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    tr = torch.empty((B, 3), dtype=torch.float32, device=dev)
    _capi.check(lib.bevamd_mat3_inverse_with_column(_capi.ptr(la), 16, 4, B, _capi.ptr(inv), _capi.ptr(tr), _capi.stream_ptr(dev)),
                "mat3_inverse_with_column")
    return inv, tr


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("cloud,mode", CASES, ids=IDS)
def test_fixture_cases_through_the_c_abi_and_the_module(dev, gold, cloud, mode):  # noqa: F811
    pts = clouds_of(gold, cloud)
    ref = dense_reference(gold, cloud, mode, pts).view(np.uint32)
    dp = [g(p, dev) for p in pts]
    keep = [p.clone() for p in dp]
    l2i, ia, la = g(gold["l2i"], dev), g(gold["ia"], dev), g(gold["la"], dev)
    inv, tr = g(gold["inv_lidar_aug_rot"], dev), g(gold["la"][:, :3, 3], dev)
    for _ in range(2):   # twice: deterministic
        got = depth_inputs(dev, dp, inv, tr, l2i, ia, IH, IW, mode_args(mode))
        assert got.shape == ref.shape and np.array_equal(bits(got), ref)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(dp, keep)), "the caller's points were changed"
    del got
    # the module on device tensors, (1) on the inverse the reference's own torch.inverse calls returned
    vt = make_module(mode, use_points="radar" if cloud == "radar" else "lidar").to(dev)
    vt.lapack_inverse = True
    real_inverse = torch.inverse

    def fixture_inverse(x):
        if tuple(x.shape) == (la.shape[0], 3, 3):
            return inv.clone()
        return real_inverse(x)

    torch.inverse = fixture_inverse
    try:
        with torch.no_grad():
            got = run_forward(vt, pts, gold, dev)      # also asserts that the caller's tensors and list are unchanged
    finally:
        torch.inverse = real_inverse
    assert np.array_equal(bits(got), ref)
    del got
    # (2) its default path == the entry point on the device-computed inverse
    vt.lapack_inverse = False
    with torch.no_grad():
        got = run_forward(vt, pts, gold, dev)
    dinv, dtr = device_inverse(dev, la)
    assert torch.equal(dtr, tr)
    exp = depth_inputs(dev, dp, dinv, dtr, l2i, ia, IH, IW, mode_args(mode))
    assert torch.equal(got.view(torch.int32), exp.view(torch.int32))
    assert all(int(m.count_nonzero()) == 0 for m in vtransforms._RASTER_MAPS.values())


def test_scalar_mode_is_the_existing_raster_and_the_map_stays_clean(dev, gold):  # noqa: F811
    """New entry, scalar mode, no features == `bevamd_depth_raster_batch`; over ONE persistent zeroed map (dense, sparse, empty cloud,
    dense again) the map is all zero after every call — with and without feature planes, and under height expansion."""
    lib = _capi.load()
    pts = clouds_of(gold, "lidar")
    l2i, ia, la = g(gold["l2i"], dev), g(gold["ia"], dev), g(gold["la"], dev)
    inv, tr = device_inverse(dev, la)
    B = len(pts)
    wsb = lib.bevamd_depth_raster_workspace_bytes(N_CAM, IH, IW) * B
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    clouds = [[g(pts[0], dev), g(pts[1], dev)], [g(pts[0][:50], dev), g(pts[1][:7], dev)], [g(pts[0][:0], dev), g(pts[1][:0], dev)],
              [g(pts[0], dev), g(pts[1], dev)]]
    for pl in clouds:
        ptrs = (ctypes.c_void_p * B)(*[p.data_ptr() for p in pl])
        counts = (ctypes.c_int * B)(*[int(p.shape[0]) for p in pl])
        exp = torch.empty((B, N_CAM, 1, IH, IW), device=dev)
        own = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _capi.check(lib.bevamd_depth_raster_batch(ptrs, counts, B, 5, _capi.ptr(inv), _capi.ptr(tr), 3, _capi.ptr(l2i), _capi.ptr(ia),
                                                  N_CAM, IH, IW, _capi.ptr(exp), _capi.ptr(own), wsb, _capi.stream_ptr(dev)),
                    "depth_raster_batch")
        for margs in ((0, 0, 0, 0), (0, 0, 0, 1), (1, 59, 1, 1)):
            got = depth_inputs(dev, pl, inv, tr, l2i, ia, IH, IW, margs, ws=ws, zero_ws=True)
            assert int(ws.count_nonzero()) == 0, margs
            other = depth_inputs(dev, pl, inv, tr, l2i, ia, IH, IW, margs)          # a map of its own, filled by the call
            assert torch.equal(got.view(torch.int32), other.view(torch.int32)), margs
            if margs[0] == 0:
                assert torch.equal(got[:, :, :1].view(torch.int32), exp.view(torch.int32)), margs
            if not pl[0].shape[0]:
                assert int(got.count_nonzero()) == 0
            del got, other
    assert int(exp.count_nonzero()) > 1000


def test_batched_call_equals_per_sample_calls_across_the_launch_limit(dev, gold):  # noqa: F811
    """17 samples (RASTER_MAX_BATCH is 16), one of them empty, on a 128x352 image with D = 30 (the output stays under 1 GB)."""
    pts = clouds_of(gold, "lidar")
    B, ih, iw, D = 17, 128, 352, 30
    pl = [g(pts[b % 2][: (0 if b == 5 else 3000 + 41 * b)], dev) for b in range(B)]
    tile = lambda a: np.concatenate([a] * 9)[:B]  # noqa: E731
    l2i, ia, la = g(tile(gold["l2i"]), dev), g(tile(gold["ia"]), dev), g(tile(gold["la"]), dev)
    inv, tr = device_inverse(dev, la)
    for margs in ((1, D, 1, 1), (0, 0, 0, 1), (1, D, 0, 0)):
        got = depth_inputs(dev, pl, inv, tr, l2i, ia, ih, iw, margs)
        for b in range(B):
            one = depth_inputs(dev, pl[b:b + 1], inv[b:b + 1].contiguous(), tr[b:b + 1].contiguous(), l2i[b:b + 1].contiguous(),
                               ia[b:b + 1].contiguous(), ih, iw, margs)
            assert torch.equal(got[b].view(torch.int32), one[0].view(torch.int32)), (margs, b)
        assert int(got[5].count_nonzero()) == 0 and int(got[16].count_nonzero()) > 100
        del got


@pytest.mark.parametrize("ih,iw,F,D,expand", [(97, 211, 3, 30, True), (64, 355, 5, 59, False), (50, 123, 18, 118, True)])
def test_random_shapes_against_the_numpy_restatement(dev, gold, ih, iw, F, D, expand):  # noqa: F811
    """Odd widths (the pixel pass leaves its 16-byte path when a plane is not a multiple of four), F = 3 / 5 / 18, D = 30 / 59 / 118."""
    rng = np.random.default_rng(ih * 1000 + iw)
    base = make_cloud("radar", 40 + F)                                  # 1 500 x 18
    pts = [np.ascontiguousarray(base[: 1500 - 100 * b, :F]) for b in range(2)]
    # bring the 256x704 projection onto the small image
    ia = gold["ia"].copy()
    scale = np.diag([iw / 704.0, ih / 256.0, 1.0, 1.0]).astype(np.float32)
    ia = (scale @ ia).astype(np.float32)
    la = gold["la"].copy()
    la[:, :3, 3] += rng.uniform(-0.2, 0.2, (2, 3)).astype(np.float32)
    l2i = gold["l2i"]
    dla = g(la, dev)
    inv, tr = device_inverse(dev, dla)
    inv_np = inv.cpu().numpy()
    dp = [g(p, dev) for p in pts]
    for depth_input, feats in (("one-hot", True), ("scalar", True), ("one-hot", False)):
        margs = mode_args(("", depth_input, expand, feats), D)
        got = depth_inputs(dev, dp, inv, tr, g(l2i, dev), g(ia, dev), ih, iw, margs).cpu().numpy()
        for b in range(2):
            exp = restate(pts[b], l2i[b], ia[b], la[b], inv_np[b], (ih, iw), depth_input, D, expand, feats)
            assert np.array_equal(got[b].view(np.uint32), exp.view(np.uint32)), (depth_input, feats, b)
        assert int((got != 0).sum()) > 200


def test_many_points_on_few_pixels(dev, gold):  # noqa: F811
    """2 cameras x (4 x 8) pixels = 64 pixels for 3 000 points (24 000 virtual ones): the winners' feature rows and the FULL bin set."""
    ih, iw, D, n_cam = 4, 8, 59, 2
    pts = [np.ascontiguousarray(make_cloud("lidar", 50 + b)[:3000]) for b in range(2)]
    scale = np.diag([iw / 704.0, ih / 256.0, 1.0, 1.0]).astype(np.float32)
    ia = (scale @ gold["ia"][:, :n_cam]).astype(np.float32)
    l2i, la = np.ascontiguousarray(gold["l2i"][:, :n_cam]), gold["la"]
    inv, tr = device_inverse(dev, g(la, dev))
    inv_np = inv.cpu().numpy()
    dp = [g(p, dev) for p in pts]
    for expand in (False, True):
        exp = [restate(pts[b], l2i[b], ia[b], la[b], inv_np[b], (ih, iw), "one-hot", D, expand, True) for b in range(2)]
        for _ in range(2):
            got = depth_inputs(dev, dp, inv, tr, g(l2i, dev), g(ia, dev), ih, iw, (1, D, int(expand), 1)).cpu().numpy()
            for b in range(2):
                assert np.array_equal(got[b].view(np.uint32), exp[b].view(np.uint32)), (expand, b)
        assert (got[:, :, :D].sum(2) >= 2).any()       # several bins on one pixel


def test_eager_equals_graph_replay(dev, gold):  # noqa: F811
    """One capture of the module's device path (one-hot + height_expand + features over the persistent map), replayed twice."""
    mode = MODES[3]
    pts = clouds_of(gold, "radar")
    vt = make_module(mode, use_points="radar").to(dev)
    dp = [g(p, dev) for p in pts]
    l2i, ia, la = g(gold["l2i"], dev), g(gold["ia"], dev), g(gold["la"], dev)
    img = torch.zeros(len(pts), N_CAM, 1, 1, 1, device=dev)
    with torch.no_grad():
        ref = vt.depth_raster(img, dp, l2i, ia, la).clone()
    static = [torch.zeros_like(p) for p in dp]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        vt.depth_raster(img, static, l2i, ia, la)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = vt.depth_raster(img, static, l2i, ia, la)
    for s, p in zip(static, dp):
        s.copy_(p)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
        out.fill_(7.0)            # the replay writes every word again
    assert all(torch.equal(a, g(p, dev)) for a, p in zip(dp, pts))
