"""GPU: the buffer contracts of the C ABI on guarded, exactly sized, dirty buffers (tests/guarded.py).

Every other GPU test hands the library `torch.empty` / `torch.zeros` buffers: the caching allocator rounds them up and parks them
among other live blocks, so a store past the end, a read of scratch the call never wrote and an output element that is never
written all go unseen.  Here every device buffer of a call — inputs, outputs, scratch, count words — is a payload of an `Arena`:
exact byte length, 64 KiB of guard on both sides, everything pre-filled with one byte.

A case is a function `run(arena) -> R`.  `drive()` checks it three ways:
  A. exact extents, twice: fill 0xFF (NaN as fp32 / fp16 / bf16, -1 as int32) and fill 0x00; scratch gets exactly the published
     size and keeps the fill (except the "must be zero" contracts); guards intact; the written parts of the outputs BIT-EQUAL
     between the fills; the parts the header leaves alone still hold the fill.
  B. against the truth: numpy / float64 / the oracle where the suite has one (with that test's tolerance, named at the case), and
     bit-equal to the same call on plain `torch.empty` buffers — what the rest of the suite pins.
  C. one byte short: `ws_bytes = published - 1` (the payload is that byte shorter too, so the guard starts there).  Either the
     call returns BEVAMD_ERR_WORKSPACE with a message and has written no output, or it is accepted and passes A and B again.
CASES maps entry points (names without the `bevamd_` prefix) to their cases; EXEMPT names the sized entry points without one.
tests/test_buffer_contracts_cover.py holds the two against the signature tables.  Importing this module does no GPU work.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from bevfusion_amd import _capi
from guarded import Arena, Plain

pytestmark = pytest.mark.gpu

ERR_WORKSPACE = 2
p = _capi.ptr


def L():
    return _capi.load()


def S(A):
    return _capi.stream_ptr(A.device)


class R:
    """What a case returns: the subject's return code, the WRITTEN parts of its outputs (name -> view), the regions the header
    says are left alone, a check against the truth (called with the outputs on the host), and — for zero-state contracts —
    a check of the scratch after the call."""

    def __init__(self, rc, out, untouched=(), ref=None, after=None):
        self.rc, self.out, self.untouched, self.ref, self.after = rc, out, list(untouched), ref, after


def _snap(out):
    return {k: v.detach().clone().cpu() for k, v in out.items()}


def _bits(t):
    t = t.contiguous()
    return t.view(-1).view(torch.uint8) if t.numel() else t.view(-1)


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, f"{what}: output {k!r}: {a[k].shape} vs {b[k].shape}"
        x, y = _bits(a[k]), _bits(b[k])
        if not torch.equal(x, y):
            bad = (x != y).nonzero().view(-1)
            raise AssertionError(f"{what}: output {k!r} differs in {bad.numel()} of {x.numel()} bytes, first at byte {int(bad[0])}, "
                                 f"last at byte {int(bad[-1])}")


def _guarded(run, dev, fill, short=0):
    A = Arena(dev, fill, short=short)
    r = run(A)
    return A, r


def _clean_run(run, dev, fill, short=0):
    """One accepted run in a guarded arena: guards, untouched regions, zero-state scratch; returns the outputs on the host."""
    A, r = _guarded(run, dev, fill, short)
    assert r.rc == 0, f"fill {fill:#04x}: code {r.rc}: {_capi.last_error()}"
    A.check()
    for v in r.untouched:
        A.untouched(v)
    if r.after is not None:
        r.after()
    return A, r, _snap(r.out)


def drive(run, dev):
    """Checks A, B and C of one case; returns (published scratch bytes, outcome of C) for the record in DESIGN.md."""
    A1, r1, ff = _clean_run(run, dev, 0xFF)
    _, _, zz = _clean_run(run, dev, 0x00)
    _same(ff, zz, "fill 0xFF vs fill 0x00")
    if r1.ref is not None:
        r1.ref(zz)
    P = Plain(dev)
    rp = run(P)
    assert rp.rc == 0
    P.check()
    _same(zz, _snap(rp.out), "guarded vs plain torch.empty buffers")
    published = sum(n for _, n in A1.ws_sizes)
    if published == 0:
        return published, "no scratch"
    A, r = _guarded(run, dev, 0xFF, short=1)
    if r.rc == ERR_WORKSPACE:
        assert _capi.last_error(), "refusal without a message"
        for o in A.outs:
            A.untouched(o)
        A.check()
        return published, "refused"
    assert r.rc == 0, f"one byte short: code {r.rc}: {_capi.last_error()}"
    A.check()
    for v in r.untouched:
        A.untouched(v)
    if r.after is not None:
        r.after()
    _same(ff, _snap(r.out), "one byte short (accepted) vs the full size")
    _, _, zs = _clean_run(run, dev, 0x00, short=1)
    _same(zz, zs, "one byte short (accepted), fill 0x00 vs the full size")
    return published, "accepted"


def _np(t):
    return t.numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# primitives: numpy is the truth (tests/test_gpu_primitives.py)
# ------------------------------------------------------------------------------------------------------------------------------
def scan_case(n, single):
    x = np.random.default_rng(n + 11).integers(0, 5, n).astype(np.int32)

    def run(A):
        lib = L()
        t, o, tot = A.put(x, "in"), A.out((n,), torch.int32, "out"), A.out((1,), torch.int32, "total")
        if single:
            ws, wsb = A.ws(lib.bevamd_scan_single_pass_state_bytes(n), "state")       # left dirty: the entry clears it
            rc = lib.bevamd_exclusive_scan_u32_single_pass(p(t), p(o), n, p(tot), p(ws), wsb, S(A))
        else:
            ws, wsb = A.ws(lib.bevamd_scan_workspace_bytes(n))
            rc = lib.bevamd_exclusive_scan_u32(p(t), p(o), n, p(tot), p(ws), wsb, S(A))

        def ref(got):
            assert np.array_equal(_np(got["out"]).astype(np.int64), np.cumsum(x, dtype=np.int64) - x)
            assert int(got["total"]) == int(x.sum())
        return R(rc, dict(out=o, total=tot), ref=ref)
    return run


SCAN_N = [0, 1, 1023, 1025, 2049, 131073]


def _keys(rng, n, nbits):
    if nbits == 32:
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        keys[::3] = keys[0] if n else 0
        return keys
    return rng.integers(0, min((1 << nbits) - 1, 5000) + 1, n).astype(np.uint32)      # few distinct keys: long runs of ties


def sort_case(n, nbits):
    keys = _keys(np.random.default_rng(n + nbits), n, nbits)
    vals = np.arange(n, dtype=np.uint32)

    def run(A):
        lib = L()
        k, v = A.put(keys.view(np.int32), "keys_in"), A.put(vals.view(np.int32), "vals_in")
        ko, vo = A.out((n,), torch.int32, "keys_out"), A.out((n,), torch.int32, "vals_out")
        ws, wsb = A.ws(lib.bevamd_radix_sort_workspace_bytes(n))
        rc = lib.bevamd_radix_sort_pairs_u32(p(k), p(v), p(ko), p(vo), n, nbits, p(ws), wsb, S(A))

        def ref(got):
            order = np.argsort(keys, kind="stable")
            assert np.array_equal(_np(got["keys"]).view(np.uint32), keys[order])
            assert np.array_equal(_np(got["vals"]).view(np.uint32), vals[order])
        return R(rc, dict(keys=ko, vals=vo), ref=ref)
    return run


def segsort_case(counts, nbits):
    n = sum(counts)
    rng = np.random.default_rng(len(counts) + nbits)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if nbits == 32 else \
        rng.integers(0, min((1 << nbits) - 1, 3000) + 1, n).astype(np.uint32)
    vals = np.concatenate([np.arange(c, dtype=np.uint32) for c in counts])
    off = np.concatenate([[0], np.cumsum(counts)])

    def run(A):
        lib = L()
        cn = (ctypes.c_int * len(counts))(*counts)
        k, v = A.put(keys.view(np.int32), "keys_in"), A.put(vals.view(np.int32), "vals_in")
        ko, vo = A.out((n,), torch.int32, "keys_out"), A.out((n,), torch.int32, "vals_out")
        ws, wsb = A.ws(lib.bevamd_radix_sort_segmented_workspace_bytes(cn, len(counts)))
        rc = lib.bevamd_radix_sort_pairs_u32_segmented(p(k), p(v), p(ko), p(vo), cn, len(counts), nbits, p(ws), wsb, S(A))

        def ref(got):
            gk, gv = _np(got["keys"]).view(np.uint32), _np(got["vals"]).view(np.uint32)
            for s in range(len(counts)):
                seg = slice(off[s], off[s + 1])
                order = np.argsort(keys[seg], kind="stable")
                assert np.array_equal(gk[seg], keys[seg][order]) and np.array_equal(gv[seg], vals[seg][order])
        return R(rc, dict(keys=ko, vals=vo), ref=ref)
    return run


# ------------------------------------------------------------------------------------------------------------------------------
# iou3d: the CPU oracle is the truth; 1e-4 is the bar of tests/test_gpu_iou3d.py::test_pairwise_vs_oracle_random
# ------------------------------------------------------------------------------------------------------------------------------
def _boxes(rng, n, spread):
    c, wh = rng.uniform(-spread, spread, (n, 2)), rng.uniform(0.4, 6.0, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2, rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)


def pairwise_case(m, n, mode):
    rng = np.random.default_rng(m * 1000 + n)
    a, b = _boxes(rng, m, 8.0), _boxes(rng, n, 8.0)

    def run(A):
        lib = L()
        ta, tb, ans = A.put(a, "boxes_a"), A.put(b, "boxes_b"), A.out((m, n), torch.float32, "ans")
        fn = lib.bevamd_iou3d_boxes_iou_bev if mode == "iou" else lib.bevamd_iou3d_boxes_overlap_bev
        rc = fn(p(ta), m, p(tb), n, p(ans), S(A))

        def ref(got):
            import oracle

            assert np.max(np.abs(_np(got["ans"]) - oracle.iou3d_pairwise(a, b, mode))) <= 1e-4
        return R(rc, dict(ans=ans), ref=ref)
    return run


def nms_case(n, normal):
    b = _boxes(np.random.default_rng(n), n, 4.0)
    thr = 0.2

    def run(A):
        lib = L()
        boxes = A.put(b, "boxes")
        keep, cnt = A.out((n,), torch.int64, "keep"), A.out((1,), torch.int32, "num_out")
        ws, wsb = A.ws(lib.bevamd_iou3d_nms_workspace_bytes(n))
        rc = lib.bevamd_iou3d_nms(p(boxes), n, thr, normal, p(keep), p(cnt), None, p(ws), wsb, S(A))
        if rc:
            return R(rc, {})
        k = int(cnt.item())
        assert 0 <= k <= n

        def ref(got):
            import oracle

            want = oracle.iou3d_nms(b, thr, normal=bool(normal)) if n else np.zeros(0, np.int64)
            assert int(got["num_out"]) == len(want) and np.array_equal(_np(got["keep"]), want)
        return R(rc, dict(keep=keep[:k], num_out=cnt), ref=ref)
    return run


# ------------------------------------------------------------------------------------------------------------------------------
# bev_pool: one plan on a 1 x 1 x 7 x 5 grid, 1001 rows = 1 camera x 7 depth bins x 11 x 13 pixels, some out of range
# ------------------------------------------------------------------------------------------------------------------------------
PB, PD, PH, PW, PN = 1, 1, 7, 5, 1001
PCELLS = PB * PD * PH * PW
FD, FH, FW = 7, 11, 13


def _pool_coords():
    rng = np.random.default_rng(5)
    c = np.stack([rng.integers(-1, PH + 1, PN), rng.integers(-1, PW + 1, PN), (rng.random(PN) < 0.05).astype(np.int64),
                  np.zeros(PN, np.int64)], 1)
    c[: PN // 4, 0], c[: PN // 4, 1] = 3, 2              # a hot cell; cell (0, 0) stays a normal one, some cells stay empty
    c[(c[:, 0] == 6) & (c[:, 1] == 4)] = (-1, 0, 0, 0)
    return c


def prepare_case(i64):
    coords = _pool_coords().astype(np.int64 if i64 else np.int32)
    cap = min(PN, PCELLS)

    def run(A):
        lib = L()
        c = A.put(coords, "coords")
        ranks, order = A.out((PN,), torch.int32, "ranks_sorted"), A.out((PN,), torch.int32, "order")
        cs = A.out((PCELLS + 2,), torch.int32, "cell_start")
        ist, iln = A.out((cap,), torch.int32, "interval_starts"), A.out((cap,), torch.int32, "interval_lengths")
        ni, geom = A.out((1,), torch.int32, "n_intervals"), A.out((PN, 4), torch.int32, "geom_sorted")
        ws, wsb = A.ws(lib.bevamd_bev_pool_prepare_workspace_bytes(PN, PB, PD, PH, PW))
        rc = lib.bevamd_bev_pool_prepare(p(c), int(i64), PN, PB, PD, PH, PW, p(ranks), p(order), p(cs), p(ist), p(iln), p(ni),
                                         p(geom), p(ws), wsb, S(A))
        if rc:
            return R(rc, {})
        k = int(ni.item())
        kept = int(cs[PCELLS].item())
        assert 0 < k <= cap and 0 < kept < PN

        def ref(got):
            x, y, z, b = (coords[:, i].astype(np.int64) for i in range(4))
            ok = (x >= 0) & (x < PH) & (y >= 0) & (y < PW) & (z >= 0) & (z < PD) & (b >= 0) & (b < PB)
            rank = np.where(ok, x * (PW * PD * PB) + y * (PD * PB) + z * PB + b, PCELLS)
            o = np.argsort(rank, kind="stable")
            assert np.array_equal(_np(got["ranks_sorted"]).view(np.uint32), rank[o])
            assert np.array_equal(_np(got["order"]).view(np.uint32), o)
            assert np.array_equal(_np(got["cell_start"])[: PCELLS + 1], np.searchsorted(rank[o], np.arange(PCELLS + 1)))
            starts = np.flatnonzero(np.r_[True, rank[o][1:int(ok.sum())] != rank[o][: int(ok.sum()) - 1]])
            assert np.array_equal(_np(got["interval_starts"]), starts)
            assert np.array_equal(_np(got["interval_lengths"]), np.diff(np.r_[starts, int(ok.sum())]))
            assert np.array_equal(_np(got["geom_sorted"]), coords[o][: int(ok.sum())].astype(np.int32))
        out = dict(ranks_sorted=ranks, order=order, cell_start=cs, interval_starts=ist[:k], interval_lengths=iln[:k], n_intervals=ni,
                   geom_sorted=geom[:kept])
        return R(rc, out, ref=ref)
    return run


def prepare_from_geom_case():
    rng = np.random.default_rng(6)
    lo, dx = np.array([-3.5, -2.5, -1.0], np.float32), np.array([1.0, 1.0, 2.0], np.float32)
    xyz = (rng.uniform(-0.15, 1.15, (PN, 3)) * np.array([PH, PW, PD]) * dx + lo).astype(np.float32)
    cap = min(PN, PCELLS)

    def run(A):
        lib = L()
        g = A.put(xyz, "geom_xyz")
        ranks, order = A.out((PN,), torch.int32, "ranks_sorted"), A.out((PN,), torch.int32, "order")
        cs = A.out((PCELLS + 2,), torch.int32, "cell_start")
        ist, iln = A.out((cap,), torch.int32, "interval_starts"), A.out((cap,), torch.int32, "interval_lengths")
        ni, geom = A.out((1,), torch.int32, "n_intervals"), A.out((PN, 4), torch.int32, "geom_sorted")
        ws, wsb = A.ws(lib.bevamd_bev_pool_prepare_workspace_bytes(PN, PB, PD, PH, PW))
        rc = lib.bevamd_bev_pool_prepare_from_geom(p(g), PN, PB, PD, PH, PW, _capi.floats(lo), _capi.floats(dx), p(ranks), p(order),
                                                   p(cs), p(ist), p(iln), p(ni), p(geom), p(ws), wsb, S(A))
        if rc:
            return R(rc, {})
        k, kept = int(ni.item()), int(cs[PCELLS].item())
        assert 0 < k <= cap and 0 < kept < PN
        out = dict(ranks_sorted=ranks, order=order, cell_start=cs, interval_starts=ist[:k], interval_lengths=iln[:k], n_intervals=ni,
                   geom_sorted=geom[:kept])
        return R(rc, out)
    return run


_PLAN = {}


def _plan(dev):
    """(ranks_sorted, order, cell_start) of the plan above as host arrays, from an ordinary call."""
    if "plan" not in _PLAN:
        r = prepare_case(True)(Plain(dev))
        assert r.rc == 0
        _PLAN["plan"] = tuple(r.out[k].cpu().numpy().copy() for k in ("ranks_sorted", "order", "cell_start"))
    return _PLAN["plan"]


def forward_cells_case(c, bf16):
    x = np.random.default_rng(c).standard_normal((PN, c)).astype(np.float32)

    def run(A):
        _, order, cs = _plan(A.device)
        xt = torch.from_numpy(x).to(torch.bfloat16) if bf16 else torch.from_numpy(x)
        tx, to, tc = A.put(xt, "x"), A.put(order, "order"), A.put(cs, "cell_start")
        out = A.out((PB, PD, PH, PW, c), torch.float32, "out")
        rc = L().bevamd_bev_pool_forward_cells(p(tx), int(bf16), p(to), p(tc), p(out), PN, c, PB, PD, PH, PW, S(A))

        def ref(got):
            """float64 segment sum; 1e-4 absolute is the bar of tests/test_gpu_bev_pool.py::test_full_op_matches_oracle"""
            coords = _pool_coords()
            ok = (coords[:, 0] >= 0) & (coords[:, 0] < PH) & (coords[:, 1] >= 0) & (coords[:, 1] < PW) & (coords[:, 2] < PD)
            want = np.zeros((PB, PD, PH, PW, c))
            np.add.at(want, (coords[ok, 3], coords[ok, 2], coords[ok, 0], coords[ok, 1]), xt.float().numpy().astype(np.float64)[ok])
            assert np.max(np.abs(_np(got["out"]) - want)) <= 1e-4
        return R(rc, dict(out=out), ref=ref)
    return run


def backward_case(kind, c=8):
    g = np.random.default_rng(17).standard_normal((PCELLS, c)).astype(np.float32)

    def run(A):
        lib = L()
        ranks, order, _ = _plan(A.device)
        og = A.put(g, "out_grad")
        xg = A.out((PN, c), torch.float32, "x_grad")
        if kind == "rows":
            to, tr = A.put(order, "order"), A.put(ranks, "ranks_sorted")
            rc = lib.bevamd_bev_pool_backward_rows(p(og), p(to), p(tr), p(xg), PN, c, PB, PD, PH, PW, S(A))
        else:
            cop = np.empty(PN, np.int64)
            cop[order.view(np.uint32)] = ranks.view(np.uint32)
            tc = A.put(cop.astype(np.uint32).view(np.int32), "cell_of_point")
            rc = lib.bevamd_bev_pool_backward_points(p(og), p(tc), p(xg), PN, c, PB, PD, PH, PW, S(A))

        def ref(got):
            """x_grad[i] = out_grad[cell of i], zeros for dropped rows: an exact copy"""
            cell = np.empty(PN, np.int64)
            cell[order.view(np.uint32)] = ranks.view(np.uint32)
            want = np.where((cell < PCELLS)[:, None], g[np.minimum(cell, PCELLS - 1)], 0).astype(np.float32)
            assert np.array_equal(_np(got["x_grad"]), want)
        return R(rc, dict(x_grad=xg), ref=ref)
    return run


def cell_of_point_case():
    def run(A):
        ranks, order, _ = _plan(A.device)
        to, tr = A.put(order, "order"), A.put(ranks, "ranks_sorted")
        cop = A.out((PN,), torch.int32, "cell_of_point")
        rc = L().bevamd_bev_pool_cell_of_point(p(to), p(tr), PN, p(cop), S(A))

        def ref(got):
            want = np.empty(PN, np.uint32)
            want[order.view(np.uint32)] = ranks.view(np.uint32)
            assert np.array_equal(_np(got["cell_of_point"]).view(np.uint32), want)
        return R(rc, dict(cell_of_point=cop), ref=ref)
    return run


def fused_forward_case(c=8):
    rng = np.random.default_rng(23)
    depth, ctx = rng.random(PN).astype(np.float32), rng.standard_normal((FH * FW, c)).astype(np.float32)

    def run(A):
        _, order, cs = _plan(A.device)
        td, tx, to, tc = A.put(depth, "depth"), A.put(ctx, "ctx"), A.put(order, "order"), A.put(cs, "cell_start")
        out = A.out((PB, PD, PH, PW, c), torch.float32, "out")
        rc = L().bevamd_bev_pool_fused_forward(p(td), p(tx), 0, p(to), p(tc), p(out), PN, c, FD, FH, FW, PB, PD, PH, PW, S(A))
        return R(rc, dict(out=out))
    return run


def columns_count_case():
    ncols = PN // FH

    def run(A):
        lib = L()
        ranks, order, _ = _plan(A.device)
        cop = np.empty(PN, np.uint32)
        cop[order.view(np.uint32)] = ranks.view(np.uint32)
        tc = A.put(cop.view(np.int32), "cell_of_point")
        keep, end = A.out((ncols,), torch.int32, "keep"), A.out((ncols,), torch.int32, "end")
        first, total = A.out((ncols,), torch.int32, "run_first"), A.out((1,), torch.int32, "total_runs")
        ws, wsb = A.ws(lib.bevamd_bev_pool_fused_columns_workspace_bytes(ncols, 0))
        rc = lib.bevamd_bev_pool_fused_columns_count(p(tc), PN, FD, FH, FW, PB, PD, PH, PW, p(keep), p(end), p(first), p(total), p(ws), wsb,
                                                     S(A))

        def ref(got):
            """bit h of keep: row h of the column is inside the grid; bit h of end: row h closes a run of equal cells"""
            cells = cop.reshape(1, FD, FH, FW).transpose(0, 1, 3, 2).reshape(ncols, FH).astype(np.int64)
            kept = cells < PCELLS
            nxt = np.concatenate([cells[:, 1:], np.full((ncols, 1), -1)], 1)
            closes = kept & (nxt != cells)
            bit = 1 << np.arange(FH, dtype=np.int64)
            assert np.array_equal(_np(got["keep"]).view(np.uint32), (kept * bit).sum(1))
            assert np.array_equal(_np(got["end"]).view(np.uint32), (closes * bit).sum(1))
            runs = closes.sum(1)
            assert np.array_equal(_np(got["run_first"]), np.cumsum(runs) - runs) and int(got["total_runs"]) == int(runs.sum())
        return R(rc, dict(keep=keep, end=end, run_first=first, total_runs=total), ref=ref)
    return run


def fused_schedule_case():
    def run(A):
        lib = L()
        _, order, cs = _plan(A.device)
        to, tc = A.put(order, "order"), A.put(cs, "cell_start")
        perm, cuts = A.out((PCELLS,), torch.int32, "perm"), A.out((9,), torch.int32, "xcd_start")
        ws, wsb = A.ws(lib.bevamd_bev_pool_fused_schedule_workspace_bytes(PCELLS))
        rc = lib.bevamd_bev_pool_fused_schedule(p(to), p(tc), PN, FD, FH, FW, PB, PD, PH, PW, p(perm), p(cuts), p(ws), wsb, S(A))

        def ref(got):
            assert sorted(_np(got["perm"]).tolist()) == list(range(PCELLS))
            cut = _np(got["xcd_start"])
            assert cut[0] == 0 and cut[8] == PCELLS and np.all(np.diff(cut) >= 0)
        return R(rc, dict(perm=perm, xcd_start=cuts), ref=ref)
    return run


# ------------------------------------------------------------------------------------------------------------------------------
# voxelization
# ------------------------------------------------------------------------------------------------------------------------------
VS, CR = (1.0, 1.0, 2.0), (0.0, 0.0, -2.0, 12.0, 10.0, 2.0)          # 12 x 10 x 2 = 240 cells


def _cloud(seed, n, f=4):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((n, f)).astype(np.float32)
    pts[:, :3] = rng.uniform((-1.0, -1.0, -2.5), (13.0, 11.0, 2.5), (n, 3))
    return pts


def hard_voxelize_case(max_voxels):
    n, f, mp = 3001, 4, 5
    pts = _cloud(31, n, f)

    def run(A):
        lib = L()
        t = A.put(pts, "points")
        vox, coors = A.out((max_voxels, mp, f), torch.float32, "voxels"), A.out((max_voxels, 3), torch.int32, "coors")
        npv, cnt = A.out((max_voxels,), torch.int32, "num_points_per_voxel"), A.out((1,), torch.int32, "voxel_num")
        ws, wsb = A.ws(lib.bevamd_hard_voxelize_workspace_bytes(n))
        rc = lib.bevamd_hard_voxelize(p(t), p(vox), p(coors), p(npv), _capi.floats(VS), _capi.floats(CR), mp, max_voxels, n, f, 3, 1,
                                      p(cnt), None, p(ws), wsb, S(A))
        if rc:
            return R(rc, {})
        k = int(cnt.item())
        assert (k == max_voxels) if max_voxels < 200 else (200 < k < max_voxels)

        def ref(got):
            import oracle

            v, c, m = oracle.hard_voxelize(pts, VS, CR, mp, max_voxels)[:3]
            assert int(got["voxel_num"]) == len(m)
            assert np.array_equal(_np(got["coors"]), c) and np.array_equal(_np(got["num_points_per_voxel"]), m)
            assert np.array_equal(_np(got["voxels"]), v)
        return R(rc, dict(voxels=vox[:k], coors=coors[:k], num_points_per_voxel=npv[:k], voxel_num=cnt),
                 untouched=[vox[k:], coors[k:], npv[k:]], ref=ref)
    return run


def voxelize_batch_case(entry, order, packed):
    f, mp, mv = 5, 4, 100
    clouds = [_cloud(41, 700, f), np.zeros((0, f), np.float32), _cloud(43, 60, f)]
    B = len(clouds)

    def run(A):
        lib = L()
        ts = [A.put(c, f"points{i}") if len(c) else None for i, c in enumerate(clouds)]
        ptrs, nums = _capi.pointers(ts), _capi.ints([len(c) for c in clouds])
        feats, coords = A.out((B * mv, f), torch.float32, "feats"), A.out((B * mv, 4), torch.int32, "coords4")
        npv = A.out((B * mv,), torch.int32, "num_points_per_voxel")
        counts, total = A.out((B,), torch.int32, "counts"), A.out((1,), torch.int32, "total")
        rows16 = A.out((B * mv, 8), torch.float16, "rows16") if entry == "rows16" else None
        ws, wsb = A.ws(lib.bevamd_voxelize_mean_batch_workspace_bytes(nums, B))
        head = (ptrs, nums, B, f, _capi.floats(VS), _capi.floats(CR), mp, mv, packed)
        outs = (p(feats), p(coords), p(npv), p(counts), p(total))
        tail = (*outs, p(ws), wsb, S(A))
        if entry == "ex":
            rc = lib.bevamd_voxelize_mean_batch_ex(*head, order, *tail)
        elif entry == "rows16":
            rc = lib.bevamd_voxelize_mean_batch_rows16(*head, order, *outs, p(rows16), 1, 8, p(ws), wsb, S(A))
        else:
            rc = lib.bevamd_voxelize_mean_batch(*head, *tail)
        if rc:
            return R(rc, {})
        cn = counts.cpu().tolist()
        assert cn[0] == mv and cn[1] == 0 and 0 < cn[2] < mv and int(total.item()) == sum(cn)       # capped, empty, under the cap
        out = dict(counts=counts, total=total)
        row = 0
        for b in range(B):
            lo = row if packed else b * mv
            for nm, t in (("feats", feats), ("coords4", coords), ("sizes", npv)) + ((("rows16", rows16),) if rows16 is not None else ()):
                out[f"{nm}{b}"] = t[lo:lo + cn[b]]
            row += cn[b]

        def ref(got):
            """the 16-bit rows are the fp32 means rounded once, zero padded to 8 columns (header)"""
            for b in range(B):
                want = torch.zeros((cn[b], 8), dtype=torch.float16)
                want[:, :f] = got[f"feats{b}"].to(torch.float16)
                assert torch.equal(_bits(got[f"rows16{b}"]), _bits(want))
        return R(rc, out, ref=ref if rows16 is not None else None)
    return run


def voxelize_mean_case(batch_idx=2):
    f, mp, mv = 5, 4, 100
    pts = _cloud(43, 60, f)               # the third sample of the batched cases: under the cap

    def run(A):
        lib = L()
        t = A.put(pts, "points")
        feats, coords = A.out((mv, f), torch.float32, "feats"), A.out((mv, 4), torch.int32, "coords4")
        npv, cnt = A.out((mv,), torch.int32, "num_points_per_voxel"), A.out((1,), torch.int32, "voxel_num")
        ws, wsb = A.ws(lib.bevamd_hard_voxelize_workspace_bytes(len(pts)))
        rc = lib.bevamd_voxelize_mean(p(t), p(feats), p(coords), p(npv), _capi.floats(VS), _capi.floats(CR), mp, mv, len(pts), f, batch_idx,
                                      p(cnt), p(ws), wsb, S(A))
        if rc:
            return R(rc, {})
        k = int(cnt.item())
        assert 0 < k < mv

        def ref(got):
            """header: the batched entry gives the results of one call of this entry per sample, bit for bit"""
            batch = voxelize_batch_case("plain", 0, 0)(Plain(A.device))
            assert batch.rc == 0 and int(batch.out["counts"][batch_idx]) == int(got["voxel_num"])
            for a, b in (("feats", "feats"), ("coords4", "coords4"), ("sizes", "num_points_per_voxel")):
                assert torch.equal(_bits(batch.out[f"{a}{batch_idx}"].cpu()), _bits(got[b])), a
        return R(rc, dict(feats=feats[:k], coords4=coords[:k], num_points_per_voxel=npv[:k], voxel_num=cnt), ref=ref)
    return run


# ------------------------------------------------------------------------------------------------------------------------------
# view-transform glue: the calibration of tests/golden/depth_inputs_ref.npz brought onto a 5 x 7 image, two cameras, two samples
# ------------------------------------------------------------------------------------------------------------------------------
RB, RCAM, RIH, RIW, RF = 2, 2, 5, 7, 5
_CAL = {}


def _calibration():
    if not _CAL:
        from bevfusion_amd import synth

        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_inputs_ref.npz"))
        scale = np.diag([RIW / 704.0, RIH / 256.0, 1.0, 1.0]).astype(np.float32)
        la = z["la"][:RB].astype(np.float32)
        _CAL.update(ia=np.ascontiguousarray((scale @ z["ia"][:RB, :RCAM]).astype(np.float32)),
                    l2i=np.ascontiguousarray(z["l2i"][:RB, :RCAM].astype(np.float32)),
                    inv=np.ascontiguousarray(np.linalg.inv(la[:, :3, :3].astype(np.float64)).astype(np.float32)),
                    trans=np.ascontiguousarray(la[:, :3, 3]),
                    pts=[np.ascontiguousarray(synth.lidar_points(seed=3 + b, sweeps=2)[b::131][: 300 - 9 * b, :RF]) for b in range(RB)])
    return _CAL


def raster_case(entry, margs=None):
    """entry: raster_batch | raster_batch_zero_ws | inputs_batch | inputs_batch_zero_ws; margs = (mode, bins, expand, features)"""
    zero = entry.endswith("zero_ws")

    def run(A):
        lib = L()
        cal = _calibration()
        pts = [A.put(q, f"points{b}") for b, q in enumerate(cal["pts"])]
        inv, tr, l2i, ia = (A.put(cal[k], k) for k in ("inv", "trans", "l2i", "ia"))
        cd = 1 if margs is None else lib.bevamd_depth_inputs_channels(margs[0], margs[1], RF, margs[3])
        depth = A.out((RB, RCAM, cd, RIH, RIW), torch.float32, "depth")
        ws, wsb = A.ws(RB * lib.bevamd_depth_raster_workspace_bytes(RCAM, RIH, RIW))
        if zero:
            ws.zero_()                                                   # the persistent map: zero before, zero after
        head = (_capi.pointers(pts), _capi.ints([q.shape[0] for q in pts]), RB, RF, p(inv), p(tr), 3, p(l2i), p(ia), RCAM, RIH, RIW)
        fn = getattr(lib, "bevamd_depth_" + entry)
        rc = fn(*head, *(margs or ()), p(depth), p(ws), wsb, S(A))

        def after():
            torch.cuda.synchronize(A.device)
            assert int(ws.count_nonzero()) == 0, "the persistent map is not all zero after the call"

        def ref(got):
            assert int((got["depth"] != 0).sum()) >= 8, "the case lost its meaning: (almost) no point lands on the image"
        return R(rc, dict(depth=depth), ref=ref, after=after if zero and isinstance(A, Arena) else None)
    return run


def raster_single_case(b=1):
    def run(A):
        lib = L()
        cal = _calibration()
        pts = A.put(cal["pts"][b], "points")
        inv, tr, l2i, ia = (A.put(cal[k][b], k) for k in ("inv", "trans", "l2i", "ia"))
        depth = A.out((RCAM, 1, RIH, RIW), torch.float32, "depth")
        ws, wsb = A.ws(lib.bevamd_depth_raster_workspace_bytes(RCAM, RIH, RIW))
        rc = lib.bevamd_depth_raster(p(pts), pts.shape[0], RF, p(inv), p(tr), p(l2i), p(ia), RCAM, RIH, RIW, p(depth), p(ws), wsb, S(A))

        def ref(got):
            """header: per sample the batched entry is identical to this one"""
            batch = raster_case("raster_batch")(Plain(A.device))
            assert batch.rc == 0 and torch.equal(_bits(batch.out["depth"][b].cpu()), _bits(got["depth"]))
        return R(rc, dict(depth=depth), ref=ref)
    return run


DEPTH_MODES = {"scalar_feat": (0, 0, 0, 1), "onehot": (1, 59, 0, 0), "onehot_feat": (1, 59, 0, 1), "onehot_expand_feat": (1, 59, 1, 1)}


# ------------------------------------------------------------------------------------------------------------------------------
# spconv: one voxel set, grid (9, 7, 5), two samples, 150 rows in ascending linear index
# ------------------------------------------------------------------------------------------------------------------------------
SHAPE, SB, SN = (9, 7, 5), 2, 150
SHAPE2 = (5, 4, 3)                                                        # 3x3x3, stride 2, padding 1
K27 = 27


def _voxels():
    lin = np.sort(np.random.default_rng(9).choice(SB * 9 * 7 * 5, SN, replace=False))
    b, r = lin // 315, lin % 315
    return np.stack([b, r // 35, r % 35 // 5, r % 5], 1).astype(np.int32)


def _geo(subm):
    return (_capi.ints(SHAPE), _capi.ints(SHAPE if subm else SHAPE2), _capi.ints([3, 3, 3]), _capi.ints([1] * 3 if subm else [2] * 3),
            _capi.ints([1, 1, 1]))


def rulebook_case(subm):
    idx = _voxels()

    def run(A):
        lib = L()
        ins, outs, ks, st, pad = _geo(subm)
        cap = lib.bevamd_spconv_max_outputs(SN, ks, st, int(subm))
        assert cap >= SN
        t = A.put(idx, "indices")
        oi = None if subm else A.out((cap, 4), torch.int32, "out_indices")
        nbr, cnt = A.out((K27, cap), torch.int32, "nbr"), A.out((1,), torch.int32, "num_out")
        ws, wsb = A.ws(lib.bevamd_spconv_rulebook_workspace_bytes(SN, SB, outs, int(subm)))
        rc = lib.bevamd_spconv_build_rulebook(p(t), SN, SB, ins, outs, ks, st, pad, None, int(subm), 0, p(oi), cap, p(nbr), cap, p(cnt),
                                              None, p(ws), wsb, S(A))
        if rc:
            return R(rc, {})
        m = int(cnt.item())
        assert (m == SN) if subm else (0 < m <= cap)
        out = dict(nbr=nbr[:, :m], num_out=cnt)
        if not subm:
            out["out_indices"] = oi[:m]

        def ref(got):
            """nbr[k][o] names the input row at out * stride - pad + k, found by brute force"""
            rows = {tuple(r): i for i, r in enumerate(idx.tolist())}
            oidx = idx if subm else _np(got["out_indices"])
            s = 1 if subm else 2
            want = np.full((K27, m), -1, np.int32)
            for o, (b, x, y, z) in enumerate(oidx.tolist()):
                for k in range(27):
                    want[k, o] = rows.get((b, x * s - 1 + k // 9, y * s - 1 + k // 3 % 3, z * s - 1 + k % 3), -1)
            assert np.array_equal(_np(got["nbr"]), want)
            if not subm:
                lin = ((oidx[:, 0] * SHAPE2[0] + oidx[:, 1]) * SHAPE2[1] + oidx[:, 2]) * SHAPE2[2] + oidx[:, 3]
                assert np.all(np.diff(lin) > 0) and np.all((want >= 0).any(0))
        return R(rc, out, ref=ref)
    return run


_SP = {}


def _rulebooks(dev):
    """Host copies of the SubM table [27, 150] and of the stride-2 rulebook (out_indices [m, 4], nbr [27, m]) from ordinary calls."""
    if not _SP:
        r = rulebook_case(True)(Plain(dev))
        assert r.rc == 0
        _SP["subm"] = r.out["nbr"].cpu().numpy().copy()
        r = rulebook_case(False)(Plain(dev))
        assert r.rc == 0
        _SP["out_indices"], _SP["nbr2"] = r.out["out_indices"].cpu().numpy().copy(), r.out["nbr"].cpu().numpy().copy()
    return _SP


def hash_neighbors_case():
    """bevamd_spconv_hash_index_build into exactly bevamd_spconv_hash_index_bytes, judged by the table bevamd_spconv_neighbors reads
    out of it (the slot a key lands in depends on the arrival order of the inserts; the lookups do not)."""
    idx = _voxels()

    def run(A):
        lib = L()
        ins, _, ks, st, pad = _geo(True)
        t, nd = A.put(idx, "indices"), A.put(np.array([SN], np.int32), "n_dev")
        index, nbytes = A.ws(lib.bevamd_spconv_hash_index_bytes(SN), "hash_index")
        nbr = A.out((K27, SN), torch.int32, "nbr")
        rc = lib.bevamd_spconv_hash_index_build(p(t), SN, p(nd), SB, ins, p(index), nbytes, S(A))
        if rc:
            return R(rc, {})
        rc = lib.bevamd_spconv_neighbors(p(t), SN, p(nd), SB, ins, ins, ks, st, pad, 1, 0, p(index), SN, p(nbr), SN, S(A))

        def ref(got):
            assert np.array_equal(_np(got["nbr"]), _rulebooks(A.device)["subm"])
        return R(rc, dict(nbr=nbr), ref=ref)
    return run


def downsample_case():
    idx = _voxels()

    def run(A):
        lib = L()
        ins, outs, ks, st, pad = _geo(False)
        cap = lib.bevamd_spconv_max_outputs(SN, ks, st, 0)
        t, nd = A.put(idx, "indices"), A.put(np.array([SN], np.int32), "n_dev")
        oi, cnt = A.out((cap, 4), torch.int32, "out_indices"), A.out((1,), torch.int32, "num_out")
        nbr = A.out((K27, cap), torch.int32, "nbr")
        index, nbytes = A.ws(lib.bevamd_spconv_rank_index_bytes(SB, outs), "rank_index")
        rc = lib.bevamd_spconv_downsample(p(t), SN, p(nd), SB, ins, outs, ks, st, pad, p(oi), cap, p(cnt), p(index), nbytes, p(nbr), cap,
                                          S(A))
        if rc:
            return R(rc, {})
        m = int(cnt.item())
        # the rank index is an output as well: judged by the SubM table bevamd_spconv_neighbors reads out of it
        nbr_s = A.out((K27, cap), torch.int32, "nbr_subm_of_outputs")
        one = _capi.ints([1, 1, 1])
        rc = lib.bevamd_spconv_neighbors(p(oi), cap, p(cnt), SB, outs, outs, ks, one, pad, 1, 1, p(index), 0, p(nbr_s), cap, S(A))

        def ref(got):
            sp = _rulebooks(A.device)
            assert np.array_equal(_np(got["out_indices"]), sp["out_indices"]) and np.array_equal(_np(got["nbr"]), sp["nbr2"])
            rows = {tuple(r): i for i, r in enumerate(sp["out_indices"].tolist())}
            want = np.full((K27, m), -1, np.int32)
            for o, (b, x, y, z) in enumerate(sp["out_indices"].tolist()):
                for k in range(27):
                    want[k, o] = rows.get((b, x - 1 + k // 9, y - 1 + k // 3 % 3, z - 1 + k % 3), -1)
            assert np.array_equal(_np(got["nbr_subm"]), want)
        return R(rc, dict(out_indices=oi[:m], num_out=cnt, nbr=nbr[:, :m], nbr_subm=nbr_s[:, :m]), ref=ref)
    return run


def sorted_index_case():
    idx = _voxels()

    def run(A):
        lib = L()
        t, nd = A.put(idx, "indices"), A.put(np.array([SN], np.int32), "n_dev")
        status = A.put(np.zeros(1, np.int32), "status")
        index, nbytes = A.ws(lib.bevamd_spconv_sorted_index_bytes(SN, SB, _capi.ints(SHAPE)), "sorted_index")
        rc = lib.bevamd_spconv_sorted_index_build(p(t), SN, p(nd), SB, _capi.ints(SHAPE), p(index), nbytes, p(status), S(A))
        if rc:
            return R(rc, {})
        # header: keys [n_cap] uint32, then (csrc/spconv_indice.hip: at the next multiple of 256 bytes) the x-plane directory
        off, ndir = (SN * 4 + 255) // 256 * 256, SB * SHAPE[0] + 1
        assert lib.bevamd_spconv_sorted_index_bytes(SN, SB, _capi.ints(SHAPE)) >= off + ndir * 4
        keys, directory = index[: SN * 4].view(torch.int32), index[off:off + ndir * 4].view(torch.int32)

        def ref(got):
            lin = ((idx[:, 0].astype(np.int64) * 9 + idx[:, 1]) * 7 + idx[:, 2]) * 5 + idx[:, 3]
            k = _np(got["keys"]).view(np.uint32).astype(np.int64)
            assert np.all(np.diff(k) > 0) and len(np.unique(lin)) == SN and int(got["status"]) == 0
            plane = idx[:, 0].astype(np.int64) * SHAPE[0] + idx[:, 1]
            assert np.array_equal(_np(got["directory"]), np.searchsorted(plane, np.arange(SB * SHAPE[0] + 1)))
        return R(rc, dict(keys=keys, status=status, directory=directory), ref=ref)
    return run


def pairs_case():
    def run(A):
        lib = L()
        sp = _rulebooks(A.device)
        nbr_h = sp["nbr2"]
        m = nbr_h.shape[1]
        nbr = A.put(nbr_h, "nbr")
        pairs, num = A.out((K27, 2, SN), torch.int32, "indice_pairs"), A.out((K27,), torch.int32, "indice_num")
        ws, wsb = A.ws(lib.bevamd_spconv_pairs_workspace_bytes(m, K27))
        rc = lib.bevamd_spconv_pairs_from_nbr(p(nbr), m, m, K27, p(pairs), SN, p(num), p(ws), wsb, S(A))

        def ref(got):
            want = np.full((K27, 2, SN), -1, np.int32)
            for k in range(K27):
                o = np.flatnonzero(nbr_h[k] >= 0)
                want[k, 0, : len(o)], want[k, 1, : len(o)] = nbr_h[k, o], o
                assert int(got["indice_num"][k]) == len(o)
            assert np.array_equal(_np(got["indice_pairs"]), want)
        return R(rc, dict(indice_pairs=pairs, indice_num=num), ref=ref)
    return run


def transpose_case():
    def run(A):
        nbr_h = _rulebooks(A.device)["nbr2"]
        m = nbr_h.shape[1]
        nbr, nbr_t = A.put(nbr_h, "nbr"), A.out((K27, SN), torch.int32, "nbr_t")
        rc = L().bevamd_spconv_transpose_nbr(p(nbr), m, m, K27, p(nbr_t), SN, S(A))

        def ref(got):
            want = np.full((K27, SN), -1, np.int32)
            for k in range(K27):
                o = np.flatnonzero(nbr_h[k] >= 0)
                want[k, nbr_h[k, o]] = o
            assert np.array_equal(_np(got["nbr_t"]), want)
        return R(rc, dict(nbr_t=nbr_t), ref=ref)
    return run


def dense_bev_case():
    C, pitch = 16, 24
    feats = np.random.default_rng(3).standard_normal((SN, C)).astype(np.float16)
    idx = _voxels()

    def run(A):
        lib = L()
        dev = A.device
        ti, nd = torch.from_numpy(idx).to(dev), torch.tensor([SN], dtype=torch.int32, device=dev)
        nb = lib.bevamd_spconv_hash_index_bytes(SN)
        plain = torch.empty(nb, dtype=torch.uint8, device=dev)
        _capi.check(lib.bevamd_spconv_hash_index_build(p(ti), SN, p(nd), SB, _capi.ints(SHAPE), p(plain), nb, S(A)), "hash index")
        index = A.put(plain, "hash_index")
        f = A.raw(SN * pitch * 2, "features").view(torch.float16).view(SN, pitch)         # gap columns keep the fill
        f[:, :C] = torch.from_numpy(feats).to(dev)
        out = A.out((SB, C * SHAPE[2], SHAPE[0], SHAPE[1]), torch.float16, "out")
        rc = lib.bevamd_spconv_dense_bev(p(f), 2, pitch, C, 0, p(index), SN, SB, _capi.ints(SHAPE), p(out), S(A))

        def ref(got):
            want = np.zeros((SB, C, SHAPE[2], SHAPE[0], SHAPE[1]), np.float16)
            want[idx[:, 0], :, idx[:, 3], idx[:, 1], idx[:, 2]] = feats
            assert np.array_equal(_np(got["out"]).view(np.uint16), want.reshape(SB, C * SHAPE[2], SHAPE[0], SHAPE[1]).view(np.uint16))
        return R(rc, dict(out=out), ref=ref)
    return run


def conv_tiled_case():
    cin = cout = 16
    rng = np.random.default_rng(12)
    feats = rng.standard_normal((SN, cin)).astype(np.float16)
    w = (rng.standard_normal((K27, cin, cout)) * 0.2).astype(np.float16)
    live = SN - 37

    def run(A):
        lib = L()
        dev = A.device
        ne = lib.bevamd_spconv_filter_image_elems(K27, cin, cout, 0)
        img = torch.empty(ne, dtype=torch.float16, device=dev)
        tw = torch.from_numpy(w).to(dev)
        _capi.check(lib.bevamd_spconv_make_filter_image(p(tw), 1, K27, cin, cout, 0, p(img), S(A)), "filter image")
        image = A.put(img, "image")
        f, nbr = A.put(feats, "features"), A.put(_rulebooks(dev)["subm"], "nbr")
        nd = A.put(np.array([live], np.int32), "num_out_dev")
        out = A.out((SN, cout), torch.float16, "out")
        rc = lib.bevamd_spconv_conv_forward_tiled(p(f), 1, cin, SN, p(image), p(nbr), SN, SN, p(nd), K27, cin, cout, p(out), cout, None,
                                                  None, None, None, 0, 0, 0, S(A))

        def ref(got):
            """float64 gather-GEMM; the fp16 bar of tests/test_gpu_spconv_tiled.py: 1e-3 * (1 + max|ref|), one rounding of the result"""
            nb = _rulebooks(dev)["subm"]
            want = np.zeros((live, cout))
            for k in range(K27):
                o = np.flatnonzero(nb[k, :live] >= 0)
                want[o] += feats[nb[k, o]].astype(np.float64) @ w[k].astype(np.float64)
            assert np.max(np.abs(_np(got["out"]).astype(np.float64) - want)) <= 1e-3 * (1.0 + np.abs(want).max())
        return R(rc, dict(out=out[:live]), untouched=[out[live:]], ref=ref)
    return run


def pad_cast_case():
    n, c, pitch = 151, 5, 8
    src = np.random.default_rng(8).standard_normal((n, c)).astype(np.float32)

    def run(A):
        s, dst = A.put(src, "src"), A.out((n, pitch), torch.float16, "dst")
        rc = L().bevamd_spconv_pad_cast_rows(p(s), n, c, pitch, 1, p(dst), S(A))

        def ref(got):
            want = np.zeros((n, pitch), np.float16)
            want[:, :c] = src.astype(np.float16)
            assert np.array_equal(_np(got["dst"]).view(np.uint16), want.view(np.uint16))
        return R(rc, dict(dst=dst), ref=ref)
    return run


def wgrad_case():
    cin = cout = 16
    rng = np.random.default_rng(14)
    feats, og = rng.standard_normal((SN, cin)).astype(np.float16), rng.standard_normal((SN, cout)).astype(np.float16)

    def run(A):
        lib = L()
        nb = _rulebooks(A.device)["subm"]
        f, g, nbr = A.put(feats, "features"), A.put(og, "out_grad"), A.put(nb, "nbr")
        fg = A.out((K27, cin, cout), torch.float16, "filter_grad")
        ws, wsb = A.ws(lib.bevamd_spconv_wgrad_workspace_bytes(K27, cin, cout))
        rc = lib.bevamd_spconv_conv_wgrad(p(f), p(g), 1, p(nbr), SN, SN, K27, cin, cout, p(fg), p(ws), wsb, S(A))

        def ref(got):
            """float64 sum of outer products; the fp16 bar of tests/test_gpu_spconv.py::test_filter_gradient_mfma_any_width_deterministic"""
            want = np.zeros((K27, cin, cout))
            for k in range(K27):
                o = np.flatnonzero(nb[k] >= 0)
                want[k] = feats[nb[k, o]].astype(np.float64).T @ og[o].astype(np.float64)
            assert np.max(np.abs(_np(got["filter_grad"]).astype(np.float64) - want)) <= 2e-3 * (1.0 + np.abs(want).max())
        return R(rc, dict(filter_grad=fg), ref=ref)
    return run


# ------------------------------------------------------------------------------------------------------------------------------
# training-mode BatchNorm over sparse rows, pitch c + 8: the gap columns hold the fill on the way in and on the way out
# ------------------------------------------------------------------------------------------------------------------------------
BN_TICKET_BYTES = 4352      # csrc/sparse_bn.hip: 33 ticket words, one per 128-byte line, rounded up to 256: the tail of the scratch
BN_TOL = {torch.float32: 2e-5, torch.float16: 2e-3}       # tests/test_gpu_sparse_bn.py::test_against_torch_modules


def _pitched(A, values, pitch, name):
    n, c = values.shape
    v = A.raw(n * pitch * values.element_size(), name).view(values.dtype).view(n, pitch)
    v[:, :c] = values.to(A.device)
    return v


def _bn_inputs(n, c, dtype):
    g = torch.Generator().manual_seed(n + c)
    x = (torch.randn((n, c), generator=g) * 1.7 + 0.3).to(dtype)
    return x, torch.randn((n, c), generator=g).to(dtype), torch.randn((n, c), generator=g).to(dtype)


def _bn_moments(x):
    xd = x.double()
    mean = xd.mean(0)
    return mean, 1.0 / torch.sqrt(((xd - mean) ** 2).mean(0) + 1e-3)


def _close(a, b, tol, scale=1.0):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= tol * scale * (1.0 + float(b.abs().max()))


def bn_stats_case(n, c, dtype):
    x, _, _ = _bn_inputs(n, c, dtype)
    dt = 0 if dtype == torch.float32 else 1

    def run(A):
        lib = L()
        tx = _pitched(A, x, c + 8, "x")
        mean, invstd = A.out((c,), torch.float32, "mean"), A.out((c,), torch.float32, "invstd")
        rm, rv = A.put(torch.full((c,), 0.1), "running_mean"), A.put(torch.full((c,), 0.9), "running_var")
        ws, wsb = A.ws(lib.bevamd_sparse_bn_workspace_bytes(c))
        ws.zero_()                                                        # zeroed ONCE for the three calls below
        out = {}
        for rep in range(3):
            rm.fill_(0.1), rv.fill_(0.9)
            rc = lib.bevamd_sparse_bn_stats(p(tx), dt, n, c, c + 8, 1e-3, 0.01, p(mean), p(invstd), p(rm), p(rv), p(ws), wsb, S(A))
            if rc:
                return R(rc, {})
            torch.cuda.synchronize(A.device)
            assert wsb > BN_TICKET_BYTES and int(ws[wsb - BN_TICKET_BYTES:].count_nonzero()) == 0, f"ticket words after call {rep}"
            for k, v in (("mean", mean), ("invstd", invstd), ("running_mean", rm), ("running_var", rv)):
                out[f"{k}{rep}"] = v.clone()
        for k in ("mean", "invstd", "running_mean", "running_var"):
            assert torch.equal(out[k + "0"], out[k + "1"]) and torch.equal(out[k + "0"], out[k + "2"]), f"{k}: three calls differ"

        def ref(got):
            m, s = _bn_moments(x)
            assert _close(got["mean0"], m, BN_TOL[dtype]) and _close(got["invstd0"], s, BN_TOL[dtype])
            var_u = (x.double() - m).pow(2).sum(0) / max(n - 1, 1)
            assert torch.allclose(got["running_mean0"].double(), 0.99 * 0.1 + 0.01 * m, rtol=1e-5, atol=1e-6)
            assert torch.allclose(got["running_var0"].double(), 0.99 * 0.9 + 0.01 * var_u, rtol=1e-5, atol=1e-6)
        return R(rc, out, ref=ref)
    return run


def bn_apply_case(n, c, dtype):
    x, res, _ = _bn_inputs(n, c, dtype)
    dt = 0 if dtype == torch.float32 else 1
    m64, s64 = _bn_moments(x)
    w, b = torch.linspace(0.5, 1.5, c), torch.linspace(-0.2, 0.2, c)

    def run(A):
        pitch = c + 8
        tx, tr = _pitched(A, x, pitch, "x"), _pitched(A, res, pitch, "residual")
        mean, invstd, tw, tb = A.put(m64.float(), "mean"), A.put(s64.float(), "invstd"), A.put(w, "weight"), A.put(b, "bias")
        y = A.out((n, pitch), dtype, "y")
        rc = L().bevamd_sparse_bn_apply(p(tx), dt, n, c, pitch, p(mean), p(invstd), p(tw), p(tb), p(tr), pitch, 1, p(y), pitch, S(A))

        def ref(got):
            want = torch.relu(((x.double() - m64.float().double()) * s64.float().double() * w.double() + b.double()).to(dtype).double()
                              + res.double())
            assert _close(got["y"], want, BN_TOL[dtype])
        return R(rc, dict(y=y[:, :c]), untouched=[y[:, c:]], ref=ref)
    return run


def bn_backward_case(n, c, dtype):
    x, res, dy = _bn_inputs(n, c, dtype)
    dt = 0 if dtype == torch.float32 else 1
    m64, s64 = _bn_moments(x)
    w, b = torch.linspace(0.5, 1.5, c), torch.linspace(-0.2, 0.2, c)
    y = torch.relu((x.double() - m64) * s64 * w.double() + b.double() + res.double()).to(dtype)

    def run(A):
        lib = L()
        pitch = c + 8
        tdy, ty, tx = _pitched(A, dy, pitch, "dy"), _pitched(A, y, pitch, "y"), _pitched(A, x, pitch, "x")
        mean, invstd, tw = A.put(m64.float(), "mean"), A.put(s64.float(), "invstd"), A.put(w, "weight")
        sdz, sdx = A.out((c,), torch.float32, "sum_dz"), A.out((c,), torch.float32, "sum_dz_xhat")
        dx, dres = A.out((n, pitch), dtype, "dx"), A.out((n, pitch), dtype, "d_residual")
        ws, wsb = A.ws(lib.bevamd_sparse_bn_workspace_bytes(c))
        ws.zero_()
        out = {}
        for rep in range(3):
            rc = lib.bevamd_sparse_bn_backward(p(tdy), pitch, p(ty), pitch, p(tx), pitch, dt, n, c, 1, p(mean), p(invstd), p(tw), p(sdz),
                                               p(sdx), p(dx), pitch, p(dres), pitch, p(ws), wsb, S(A))
            if rc:
                return R(rc, {})
            torch.cuda.synchronize(A.device)
            assert wsb > BN_TICKET_BYTES and int(ws[wsb - BN_TICKET_BYTES:].count_nonzero()) == 0, f"ticket words after call {rep}"
            for k, v in (("sum_dz", sdz), ("sum_dz_xhat", sdx), ("dx", dx[:, :c]), ("d_residual", dres[:, :c])):
                out[f"{k}{rep}"] = v.clone()
        for k in ("sum_dz", "sum_dz_xhat", "dx", "d_residual"):
            assert torch.equal(_bits(out[k + "0"]), _bits(out[k + "1"])) and torch.equal(_bits(out[k + "0"]), _bits(out[k + "2"])), k

        def ref(got):
            tol = BN_TOL[dtype]
            dz = dy.double() * (y.double() > 0)
            xhat = (x.double() - m64.float().double()) * s64.float().double()
            sd, sx = dz.sum(0), (dz * xhat).sum(0)
            want = w.double() * s64.float().double() * (dz - sd / n - xhat * sx / n)
            assert _close(got["sum_dz0"], sd, tol, 4.0) and _close(got["sum_dz_xhat0"], sx, tol, 4.0)
            assert _close(got["dx0"], want, tol) and _close(got["d_residual0"], dz, tol)
        return R(rc, out, untouched=[dx[:, c:], dres[:, c:]], ref=ref)
    return run


# ------------------------------------------------------------------------------------------------------------------------------
# ext library
# ------------------------------------------------------------------------------------------------------------------------------
def seg_iou_case():
    shape = (2, 3, 63)
    g = torch.Generator().manual_seed(sum(shape))
    pred = torch.rand(shape, generator=g)
    pred.view(-1)[::7], pred.view(-1)[3::11], pred.view(-1)[5::13] = float("nan"), float("inf"), -float("inf")
    label = (torch.rand(shape, generator=g) < 0.5).to(torch.uint8)
    thr = torch.tensor([i / 17 for i in range(1, 17)], dtype=torch.float32)

    def run(A):
        tp, tl, tt = A.put(pred, "pred"), A.put(label, "label"), A.put(thr, "thresholds")
        counts = A.out((shape[1], 16, 3), torch.int64, "counts")
        rc = L().bevamd_seg_iou_counts(p(tp), p(tl), 3, shape[0], shape[1], shape[2], p(tt), 16, p(counts), S(A))

        def ref(got):
            pr = pred.permute(1, 0, 2).reshape(shape[1], 1, -1) >= thr.view(1, -1, 1)
            lb = label.bool().permute(1, 0, 2).reshape(shape[1], 1, -1)
            want = torch.stack([(pr & lb).sum(-1), (pr & ~lb).sum(-1), (~pr & lb).sum(-1)], -1)
            assert torch.equal(got["counts"], want)
        return R(rc, dict(counts=counts), ref=ref)
    return run


def _qkv(B, H, Lq, Sk):
    g = torch.Generator().manual_seed(B * 1000 + Sk)
    return (torch.randn((B, Lq, H * 16), generator=g), torch.randn((B, Sk, H * 16), generator=g), torch.randn((B, Sk, H * 16), generator=g),
            torch.randn((B, Lq, H * 16), generator=g))


def mha_forward_case(B, H, Lq, Sk, with_stats):
    q, k, v, _ = _qkv(B, H, Lq, Sk)

    def run(A):
        lib = L()
        tq, tk, tv = A.put(q, "q"), A.put(k, "k"), A.put(v, "v")
        out, lse = A.out((B, Lq, H * 16), torch.float32, "out"), A.out((B, H, Lq), torch.float32, "lse")
        stats = A.out((2, B, H, Lq), torch.float32, "stats") if with_stats else None
        ws, wsb = A.ws(lib.bevamd_mha_workspace_bytes(B, H, Lq, Sk))
        rc = lib.bevamd_mha_forward(p(tq), p(tk), p(tv), B, H, Lq, Sk, 0, 0.0, 0, p(out), p(lse), p(stats), p(ws), wsb, S(A))

        o = dict(out=out, lse=lse)
        if with_stats:
            o["stats"] = stats
        return R(rc, o)       # header: equal calls are bit-equal; tests/test_gpu_decoder_layer.py pins the plain call's values
    return run


def mha_backward_case(B, H, Lq, Sk):
    q, k, v, dout = _qkv(B, H, Lq, Sk)

    def run(A):
        lib = L()
        dev = A.device
        fwd = mha_forward_case(B, H, Lq, Sk, True)(Plain(dev))
        assert fwd.rc == 0
        tq, tk, tv, tdo = A.put(q, "q"), A.put(k, "k"), A.put(v, "v"), A.put(dout, "dout")
        to, ts = A.put(fwd.out["out"], "out"), A.put(fwd.out["stats"], "stats")
        dq, dk, dv = A.out(q.shape, torch.float32, "dq"), A.out(k.shape, torch.float32, "dk"), A.out(v.shape, torch.float32, "dv")
        ws, wsb = A.ws(lib.bevamd_mha_workspace_bytes(B, H, Lq, Sk))
        rc = lib.bevamd_mha_backward(p(tq), p(tk), p(tv), p(to), p(ts), p(tdo), B, H, Lq, Sk, 0.0, 0, p(dq), p(dk), p(dv), p(ws), wsb, S(A))

        return R(rc, dict(dq=dq, dk=dk, dv=dv))
    return run


def head_proposals_case():
    B, C, H, W, K, ks = 2, 3, 7, 3, 5, 3
    logits = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(77))

    def run(A):
        lib = L()
        t = A.put(logits, "logits")
        cls, idx = A.out((B, K), torch.int64, "top_class"), A.out((B, K), torch.int64, "top_index")
        score = A.out((B, K), torch.float32, "top_score")
        ws, wsb = A.ws(lib.bevamd_head_proposals_workspace_bytes(B, C, H, W))
        rc = lib.bevamd_head_proposals(p(t), B, C, H, W, ks, 0, K, p(cls), p(idx), p(score), p(ws), wsb, S(A))

        def ref(got):
            """local maxima of the sigmoid off the border, stable descending order (the header's definition)"""
            s = torch.sigmoid(logits.double())
            keep = torch.zeros_like(s)
            inner = torch.nn.functional.max_pool2d(s, ks, stride=1, padding=0)
            keep[:, :, 1:-1, 1:-1] = inner
            s = s * (s == keep)
            flat = s.view(B, -1)
            top = torch.argsort(-flat, dim=1, stable=True)[:, :K]
            assert torch.equal(got["top_class"], top // (H * W)) and torch.equal(got["top_index"], top % (H * W))
        return R(rc, dict(top_class=cls, top_index=idx, top_score=score), ref=ref)
    return run


def centerpoint_select_case():
    B, H, W, K, classes = 2, 8, 8, 5, [1, 2]
    g = torch.Generator().manual_seed(78)
    heats = [torch.randn((B, c, H, W), generator=g) for c in classes]

    def run(A):
        lib = L()
        ts = [A.put(h, f"heatmap{i}") for i, h in enumerate(heats)]
        flat, score = A.out((B, 2, K), torch.int32, "top_flat"), A.out((B, 2, K), torch.float32, "top_score")
        ws, wsb = A.ws(lib.bevamd_centerpoint_select_workspace_bytes(B, sum(classes), H, W))
        rc = lib.bevamd_centerpoint_select(_capi.pointers(ts), _capi.ints(classes), 2, B, H, W, K, 1, p(flat), p(score), p(ws), wsb, S(A))

        def ref(got):
            for t, h in enumerate(heats):
                top = torch.argsort(-h.reshape(B, -1), dim=1, stable=True)[:, :K]          # sigmoid is monotonic: same order
                assert torch.equal(got["top_flat"][:, t].long(), top)
        return R(rc, dict(top_flat=flat, top_score=score), ref=ref)
    return run


def scatter_index_case():
    n, ndim = 257, 3
    rng = np.random.default_rng(257)
    coors = rng.integers(-1, 6, (n, ndim)).astype(np.int32)

    def run(A):
        lib = L()
        t = A.put(coors, "coors")
        oc, cmap = A.out((n, ndim), torch.int32, "out_coors"), A.out((n,), torch.int32, "coors_map")
        cnt, order, seg = A.out((n,), torch.int32, "reduce_count"), A.out((n,), torch.int32, "order"), A.out((n + 1,), torch.int32, "seg_start")
        mdev = A.out((1,), torch.int32, "num_voxels")
        ws, wsb = A.ws(lib.bevamd_dynamic_scatter_workspace_bytes(n))
        rc = lib.bevamd_dynamic_scatter_index(p(t), n, ndim, p(oc), p(cmap), p(cnt), p(order), p(seg), p(mdev), None, p(ws), wsb, S(A))
        if rc:
            return R(rc, {})
        m = int(mdev.item())
        kept = int((coors >= 0).all(1).sum())
        assert 0 < m < n

        def ref(got):
            ok = (coors >= 0).all(1)
            uniq, inv, c = np.unique(coors[ok], axis=0, return_inverse=True, return_counts=True)
            want_map = np.full(n, -1, np.int32)
            want_map[ok] = inv.reshape(-1)
            assert int(got["num_voxels"]) == len(uniq) and np.array_equal(_np(got["out_coors"]), uniq)
            assert np.array_equal(_np(got["coors_map"]), want_map) and np.array_equal(_np(got["reduce_count"]), c)
            o = np.flatnonzero(ok)[np.argsort(inv.reshape(-1), kind="stable")]
            assert np.array_equal(_np(got["order"]), o) and np.array_equal(_np(got["seg_start"]), np.r_[0, np.cumsum(c)])
        return R(rc, dict(out_coors=oc[:m], coors_map=cmap, reduce_count=cnt[:m], order=order[:kept], seg_start=seg[:m + 1], num_voxels=mdev),
                 untouched=[oc[m:], cnt[m:]], ref=ref)
    return run


# ------------------------------------------------------------------------------------------------------------------------------
# the registry
# ------------------------------------------------------------------------------------------------------------------------------
F16, F32 = torch.float16, torch.float32
BN_SHAPES = [(5, 16, F16), (5, 16, F32), (333, 8, F16), (333, 8, F32)]
MHA_SHAPES = [(3, 2, 15, 17), (1, 8, 17, 64 + 1)]            # decoder.SPLIT_KEYS_MIN + 1 keys: two forward splits


def _bn_id(n, c, dt):
    return f"{n}x{c}-{'fp16' if dt == F16 else 'fp32'}"


CASES = {
    # sized entry points (a pointer followed by its byte count)
    "exclusive_scan_u32": [(str(n), scan_case(n, False)) for n in SCAN_N],
    "exclusive_scan_u32_single_pass": [(str(n), scan_case(n, True)) for n in SCAN_N],
    "radix_sort_pairs_u32": [(f"{n}-{b}bit", sort_case(n, b)) for n, b in [(1, 8), (4095, 17), (4097, 20), (100003, 32)]],
    "radix_sort_pairs_u32_segmented": [(f"{len(c)}seg-{b}bit", segsort_case(c, b)) for c, b in
                                       [([1023, 1025], 32), ([0, 0, 70000], 27), ([0, 70000, 0, 0, 1, 2, 3, 1024, 50000], 20)]],
    "iou3d_nms": [(f"{n}-{'normal' if nm else 'rotated'}", nms_case(n, nm)) for n in (0, 1, 63, 65, 129) for nm in (0, 1)],
    "bev_pool_prepare": [("int64", prepare_case(True)), ("int32", prepare_case(False))],
    "bev_pool_prepare_from_geom": [("geom", prepare_from_geom_case())],
    "bev_pool_fused_schedule": [("plan", fused_schedule_case())],
    "bev_pool_fused_columns_count": [("plan", columns_count_case())],
    "hard_voxelize": [("capped", hard_voxelize_case(50)), ("rows_left", hard_voxelize_case(500))],
    "voxelize_mean_batch_ex": [(f"order{o}-packed{k}", voxelize_batch_case("ex", o, k)) for o in (0, 1) for k in (0, 1)],
    "voxelize_mean": [("60", voxelize_mean_case())],
    "voxelize_mean_batch_rows16": [(f"order{o}-packed{k}", voxelize_batch_case("rows16", o, k)) for o, k in ((0, 0), (1, 1))],
    "voxelize_mean_batch": [(f"packed{k}", voxelize_batch_case("plain", 0, k)) for k in (0, 1)],
    "depth_raster": [("2x5x7", raster_single_case())],
    "depth_raster_batch": [("2x2x5x7", raster_case("raster_batch"))],
    "depth_raster_batch_zero_ws": [("2x2x5x7", raster_case("raster_batch_zero_ws"))],
    "depth_inputs_batch": [(k, raster_case("inputs_batch", m)) for k, m in DEPTH_MODES.items()],
    "depth_inputs_batch_zero_ws": [(k, raster_case("inputs_batch_zero_ws", m)) for k, m in DEPTH_MODES.items()],
    "spconv_build_rulebook": [("subm", rulebook_case(True)), ("stride2", rulebook_case(False))],
    "spconv_hash_index_build": [("neighbors", hash_neighbors_case())],
    "spconv_downsample": [("with_nbr", downsample_case())],
    "spconv_sorted_index_build": [("150", sorted_index_case())],
    "spconv_pairs_from_nbr": [("stride2", pairs_case())],
    "spconv_conv_wgrad": [("fp16-16x16", wgrad_case())],
    "sparse_bn_stats": [(_bn_id(*s), bn_stats_case(*s)) for s in BN_SHAPES],
    "sparse_bn_backward": [(_bn_id(*s), bn_backward_case(*s)) for s in BN_SHAPES],
    "mha_forward": [(f"{'x'.join(map(str, s))}-{'stats' if st else 'nostats'}", mha_forward_case(*s, st)) for s in MHA_SHAPES
                    for st in (True, False)],
    "mha_backward": [("x".join(map(str, s)), mha_backward_case(*s)) for s in MHA_SHAPES],
    "head_proposals": [("2x3x7x3", head_proposals_case())],
    "centerpoint_select": [("2x3x8x8", centerpoint_select_case())],
    "dynamic_scatter_index": [("257", scatter_index_case())],
    # entry points without scratch whose header promises extents
    "iou3d_boxes_iou_bev": [(f"{m}x{n}", pairwise_case(m, n, "iou")) for m, n in [(1, 1), (3, 65), (5, 127)]],
    "iou3d_boxes_overlap_bev": [(f"{m}x{n}", pairwise_case(m, n, "overlap")) for m, n in [(1, 1), (3, 65), (5, 127)]],
    "bev_pool_forward_cells": [(f"c{c}-{'bf16' if bf else 'fp32'}", forward_cells_case(c, bf)) for c in (1, 80) for bf in (False, True)],
    "bev_pool_backward_rows": [("c8", backward_case("rows"))],
    "bev_pool_backward_points": [("c8", backward_case("points"))],
    "bev_pool_cell_of_point": [("plan", cell_of_point_case())],
    "bev_pool_fused_forward": [("c8", fused_forward_case())],
    "spconv_conv_forward_tiled": [("fp16-16x16-device-count", conv_tiled_case())],
    "spconv_transpose_nbr": [("stride2", transpose_case())],
    "spconv_dense_bev": [("fp16-pitch24", dense_bev_case())],
    "spconv_pad_cast_rows": [("151x5", pad_cast_case())],
    "sparse_bn_apply": [(_bn_id(*s), bn_apply_case(*s)) for s in BN_SHAPES],
    "seg_iou_counts": [("2x3x63", seg_iou_case())],
}

EXEMPT = {
    "bev_pool_fused_columns_build": "needs the run counts of a column plan read back; tests/test_gpu_fused_columns.py builds them",
    "spconv_downsample_sorted": "needs the x-plane directory of a sorted-key index as input; covered through spconv_downsample's output set",
    "spconv_conv_wgrad_slab": "needs slab metadata in the baked filter-gradient format; tests/test_gpu_wgrad_slab.py builds it",
}

# the size function of every covered sized entry at its tested shape, callable without a device (tests/test_buffer_contracts_cover.py)
PUBLISHED = {
    "exclusive_scan_u32": lambda lib: lib.bevamd_scan_workspace_bytes(1025),
    "exclusive_scan_u32_single_pass": lambda lib: lib.bevamd_scan_single_pass_state_bytes(1025),
    "radix_sort_pairs_u32": lambda lib: lib.bevamd_radix_sort_workspace_bytes(4097),
    "radix_sort_pairs_u32_segmented": lambda lib: lib.bevamd_radix_sort_segmented_workspace_bytes(_capi.ints([1023, 1025]), 2),
    "iou3d_nms": lambda lib: lib.bevamd_iou3d_nms_workspace_bytes(129),
    "bev_pool_prepare": lambda lib: lib.bevamd_bev_pool_prepare_workspace_bytes(PN, PB, PD, PH, PW),
    "bev_pool_prepare_from_geom": lambda lib: lib.bevamd_bev_pool_prepare_workspace_bytes(PN, PB, PD, PH, PW),
    "bev_pool_fused_schedule": lambda lib: lib.bevamd_bev_pool_fused_schedule_workspace_bytes(PCELLS),
    "bev_pool_fused_columns_count": lambda lib: lib.bevamd_bev_pool_fused_columns_workspace_bytes(PN // FH, 0),
    "hard_voxelize": lambda lib: lib.bevamd_hard_voxelize_workspace_bytes(3001),
    "voxelize_mean_batch_ex": lambda lib: lib.bevamd_voxelize_mean_batch_workspace_bytes(_capi.ints([700, 0, 60]), 3),
    "voxelize_mean": lambda lib: lib.bevamd_hard_voxelize_workspace_bytes(60),
    "voxelize_mean_batch_rows16": lambda lib: lib.bevamd_voxelize_mean_batch_workspace_bytes(_capi.ints([700, 0, 60]), 3),
    "voxelize_mean_batch": lambda lib: lib.bevamd_voxelize_mean_batch_workspace_bytes(_capi.ints([700, 0, 60]), 3),
    "depth_raster": lambda lib: lib.bevamd_depth_raster_workspace_bytes(RCAM, RIH, RIW),
    "depth_raster_batch": lambda lib: RB * lib.bevamd_depth_raster_workspace_bytes(RCAM, RIH, RIW),
    "depth_raster_batch_zero_ws": lambda lib: RB * lib.bevamd_depth_raster_workspace_bytes(RCAM, RIH, RIW),
    "depth_inputs_batch": lambda lib: RB * lib.bevamd_depth_raster_workspace_bytes(RCAM, RIH, RIW),
    "depth_inputs_batch_zero_ws": lambda lib: RB * lib.bevamd_depth_raster_workspace_bytes(RCAM, RIH, RIW),
    "spconv_build_rulebook": lambda lib: lib.bevamd_spconv_rulebook_workspace_bytes(SN, SB, _capi.ints(SHAPE2), 0),
    "spconv_hash_index_build": lambda lib: lib.bevamd_spconv_hash_index_bytes(SN),
    "spconv_downsample": lambda lib: lib.bevamd_spconv_rank_index_bytes(SB, _capi.ints(SHAPE2)),
    "spconv_sorted_index_build": lambda lib: lib.bevamd_spconv_sorted_index_bytes(SN, SB, _capi.ints(SHAPE)),
    "spconv_pairs_from_nbr": lambda lib: lib.bevamd_spconv_pairs_workspace_bytes(SN, K27),
    "spconv_conv_wgrad": lambda lib: lib.bevamd_spconv_wgrad_workspace_bytes(K27, 16, 16),
    "sparse_bn_stats": lambda lib: lib.bevamd_sparse_bn_workspace_bytes(16),
    "sparse_bn_backward": lambda lib: lib.bevamd_sparse_bn_workspace_bytes(16),
    "mha_forward": lambda lib: lib.bevamd_mha_workspace_bytes(3, 2, 15, 17),
    "mha_backward": lambda lib: lib.bevamd_mha_workspace_bytes(3, 2, 15, 17),
    "head_proposals": lambda lib: lib.bevamd_head_proposals_workspace_bytes(2, 3, 7, 3),
    "centerpoint_select": lambda lib: lib.bevamd_centerpoint_select_workspace_bytes(2, 3, 8, 8),
    "dynamic_scatter_index": lambda lib: lib.bevamd_dynamic_scatter_workspace_bytes(257),
}

PARAMS = [pytest.param(name, run, id=f"{name}-{cid}") for name, cases in CASES.items() for cid, run in cases]


@pytest.mark.parametrize("name,run", PARAMS)
def test_buffer_contract(dev, name, run):
    published, outcome = drive(run, dev)
    assert name in PUBLISHED or published == 0
    assert outcome in ("refused", "accepted", "no scratch")
