"""GPU: the TransFusion assignment kernels (csrc/ext/head_assign.hip).

The solver alone, against scipy on the same matrix read back: exact rows where the optimum is unique almost surely (seeded
continuous costs), validity and totals where it is not (integer costs, an all-equal matrix), the long-augmenting-path matrix,
per-problem live sizes with NaN padding, and non-finite entries (the return is checked: the kernel's loops are bounded by
construction, see the header of the unit).  Totals bar: 1e-9 * max(1, |total|): both matchings are optimal for the same fp32 matrix,
so their float64 totals differ only by the fp64 rounding of at most ~10^3 dual updates.

The full path, against tests/golden/head_assign_ref.npz under the bars of tests/test_head_assign.py.  The cost / iou bar is twice
the largest absolute error observed on an MI355X, committed in profiles/head_assign_parity_observed.json; the test asserts
2 * min(K, G) * bar < margin for every row-wise fixture, which is what makes the golden's unique optimum the optimum on the
device's costs too, so that comparing rows exactly is legitimate.  `config_shape` has no unique optimum and is checked by validity,
by its totals against scipy ON THE DEVICE'S OWN cost matrix, and by the targets the host mirror derives from the device's own
assignment."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import iou3d_families as families
import oracle
from bevfusion_amd import head_assign, head_targets, heads
from conftest import record_parity
from test_head_assign import (CASES, ROWWISE, check_targets, cost_errors, gen, gold, host_mirror, make_assigner, make_coder,  # noqa: F401
                              margin_admits)
from test_head_targets import check_heatmap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("labels", "label_weights", "bbox_targets", "bbox_weights", "ious", "num_pos", "matched_ious", "heatmap", "flags")


@pytest.fixture(scope="module")
def bars():
    """Twice the largest absolute error observed on the device (the committed measurement)."""
    with open(os.path.join(ROOT, "profiles", "head_assign_parity_observed.json")) as fh:
        seen = json.load(fh)
    return 2 * float(seen["cost_abs_err_observed"]), 2 * float(seen["iou_abs_err_observed"])


# ---- the solver alone ------------------------------------------------------------------------------------------------------------
def solve(cost, dev, rows=None, cols=None):
    t = torch.from_numpy(np.ascontiguousarray(cost)).to(dev)
    to = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    col4row, status = heads.linear_sum_assignment_batch(t, to(rows), to(cols))
    return col4row.cpu().numpy(), status.cpu().numpy()


def scipy_rows(cost):
    r, c = linear_sum_assignment(cost)
    out = np.full(cost.shape[0], -1, np.int32)
    out[r] = c
    return out


def total_of(cost, col4row):
    rows = np.nonzero(col4row >= 0)[0]
    return cost[rows, col4row[rows]].astype(np.float64).sum()


def check_valid(col4row, nr, nc):
    live = col4row[:nr]
    matched = live[live >= 0]
    assert (col4row[nr:] == -1).all() and len(matched) == min(nr, nc) and len(set(matched.tolist())) == len(matched)
    assert (matched < nc).all()


SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (13, 8), (8, 13), (63, 65), (64, 64), (65, 63), (200, 40), (40, 200)]


def test_solver_matches_scipy_on_continuous_costs(dev):
    rng = np.random.default_rng(4100)
    for r, c in SHAPES:
        cost = rng.uniform(-1, 1, (3, r, c)).astype(np.float32)
        got, status = solve(cost, dev)
        assert not status.any()
        for n in range(3):
            assert np.array_equal(got[n], scipy_rows(cost[n])), (r, c, n)


def test_solver_largest_problem(dev):
    cost = np.random.default_rng(4101).uniform(0, 1, (1024, 1024)).astype(np.float32)
    got, status = solve(cost, dev)
    assert status == 0 and np.array_equal(got, scipy_rows(cost))


@pytest.mark.parametrize("kind", ["integers", "all_equal"])
def test_solver_ties_totals_and_validity(kind, dev):
    rng = np.random.default_rng(4102)
    for r, c in [(13, 8), (8, 13), (64, 64), (200, 40), (40, 200), (65, 63)]:
        cost = rng.integers(0, 4, (2, r, c)).astype(np.float32) if kind == "integers" else np.full((2, r, c), 0.37, np.float32)
        got, status = solve(cost, dev)
        assert not status.any()
        for n in range(2):
            check_valid(got[n], r, c)
            want = total_of(cost[n], scipy_rows(cost[n]))
            assert abs(total_of(cost[n], got[n]) - want) <= 1e-9 * max(1.0, abs(want)), (kind, r, c)


def test_solver_long_augmenting_paths(dev):
    i = np.arange(1, 65, dtype=np.float64)
    cost = (i[:, None] * i[None, :]).astype(np.float32)
    got, status = solve(cost, dev)
    check_valid(got, 64, 64)
    want = total_of(cost, scipy_rows(cost))
    assert status == 0 and abs(total_of(cost, got) - want) <= 1e-9 * max(1.0, abs(want))
    assert np.array_equal(got, scipy_rows(cost))                           # the anti-diagonal: unique by the rearrangement inequality


def test_solver_live_sizes_from_device_memory(dev):
    """Per-problem live sizes smaller than the buffer; the padding is NaN and must never be read."""
    rng = np.random.default_rng(4103)
    sizes = [(5, 9), (20, 3), (1, 1), (24, 16), (0, 7), (7, 0), (17, 17)]
    cost = np.full((len(sizes), 24, 17), np.nan, np.float32)
    for n, (r, c) in enumerate(sizes):
        cost[n, :r, :c] = rng.uniform(-3, 3, (r, c))
    got, status = solve(cost, dev, rows=[s[0] for s in sizes], cols=[s[1] for s in sizes])
    assert not status.any()
    for n, (r, c) in enumerate(sizes):
        check_valid(got[n], r, c)
        if r and c:
            assert np.array_equal(got[n, :r], scipy_rows(cost[n, :r, :c]))


def test_solver_rejects_non_finite_entries_and_spares_the_neighbours(dev):
    rng = np.random.default_rng(4104)
    cost = rng.uniform(0, 1, (5, 12, 9)).astype(np.float32)
    cost[1, 3, 4] = np.nan
    cost[3, 11, 8] = np.inf
    cost[4, 0, 0] = -np.inf
    got, status = solve(cost, dev)
    assert status.tolist() == [0, head_assign.STATUS_NONFINITE, 0, head_assign.STATUS_NONFINITE, head_assign.STATUS_NONFINITE]
    assert (got[[1, 3, 4]] == -1).all()
    for n in (0, 2):
        assert np.array_equal(got[n], scipy_rows(cost[n]))
    got, status = solve(cost[:2], dev, rows=[12, 40], cols=[9, 9])         # a live size outside the buffer
    assert status.tolist() == [0, head_assign.STATUS_BOUND] and (got[1] == -1).all() and np.array_equal(got[0], scipy_rows(cost[0]))


# ---- the full path ---------------------------------------------------------------------------------------------------------------
def device_inputs(case, dev, form):
    d = gen.inputs(case)
    preds = {k: torch.from_numpy(v).to(dev) for k, v in d["preds"].items()}
    if form == "lists":
        gt = ([torch.from_numpy(b).to(dev) for b in d["gt_boxes"]], [torch.from_numpy(l).to(dev) for l in d["gt_labels"]])
        kw = {}
    else:
        gt = (tuple(torch.from_numpy(a).to(dev) for a in gen.packed(case)), None)
        kw = dict(max_boxes_per_sample=max(max(gen.CASES[case]["G"]), 1) + 3)
    return preds, gt, kw


def get_targets(case, dev, form="lists", sync=False, **over):
    c = gen.CASES[case]
    preds, gt, kw = device_inputs(case, dev, form)
    kw.update(over)
    return heads.transfusion_get_targets(*gt, preds, make_coder(case), make_assigner(case), gen.case_cfg(case), c["K"], gen.C,
                                         num_decoder_layers=c["L"], sync=sync, **kw)


def as_dict(out):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in zip(NAMES, out)}


def device_costs(case, dev):
    """(cost, iou [B, L, K, Gmax], col4row, status words) of the device path on a fixture."""
    c = gen.CASES[case]
    preds, gt, _ = device_inputs(case, dev, "lists")
    packed = head_targets._pack(*gt, None)
    boxes = heads._decode_device(preds["heatmap"], preds["rot"], preds["dim"], preds["center"], preds["height"], preds.get("vel"),
                                 make_coder(case), c["L"] * c["K"])[0]
    cost, iou, col4row, st_cost, st_lsa = make_assigner(case)._solve(boxes, preds["heatmap"], packed[:3], c["L"], c["K"], packed[4],
                                                                     gen.case_cfg(case))
    return cost.cpu().numpy(), iou.cpu().numpy(), col4row.cpu().numpy(), st_cost.cpu().numpy(), st_lsa.cpu().numpy(), boxes.cpu().numpy()


@pytest.mark.parametrize("case", ROWWISE)
def test_costs_match_the_reference(case, gold, bars, dev):
    cost, iou, col4row, st_cost, st_lsa, _ = device_costs(case, dev)
    ec, ei = cost_errors(case, gold, cost, iou)
    print(f"{case}: cost error {ec:.3e} (bar {bars[0]:.3e}), iou error {ei:.3e} (bar {bars[1]:.3e}), margin {float(gold[case + '.margin']):.3e}")
    record_parity(f"head_assign/{case}/cost_abs_err", ec, bars[0])
    record_parity(f"head_assign/{case}/iou_abs_err", ei, bars[1])
    assert margin_admits(case, gold, bars[0])
    assert ec <= bars[0] and ei <= bars[1]
    assert not st_cost.any() and not st_lsa.any()
    assert np.array_equal(col4row, gold[case + ".col4row"])
    for b, G in enumerate(gen.CASES[case]["G"]):                           # slots past the live count are written as zeros
        assert not cost[b, :, :, G:].any() and not iou[b, :, :, G:].any()


@pytest.mark.parametrize("form", ["lists", "packed"])
@pytest.mark.parametrize("case", ROWWISE)
def test_targets_match_the_reference(case, form, gold, bars, dev):
    assert margin_admits(case, gold, bars[0])
    got = as_dict(get_targets(case, dev, form))
    err, mean_err = check_targets(case, gold, got, bars[1])
    record_parity(f"head_assign/{case}/{form}/ious_abs_err", max(err, mean_err), bars[1])
    assert not got["flags"].any() and got["num_pos"].dtype == np.int32 and got["matched_ious"].dtype == np.float32
    gt_boxes, gt_labels, offsets = gen.packed(case)
    want_heat, _ = head_targets._targets_host(gt_boxes, gt_labels, offsets, gen.C, gen.case_cfg(case))
    assert check_heatmap(got["heatmap"], want_heat) == 0
    synced = get_targets(case, dev, form, sync=True)                        # the reference's own 8-tuple
    assert len(synced) == 8 and type(synced[5]) is int and type(synced[6]) is float
    assert synced[5] == int(got["num_pos"]) and np.float32(synced[6]) == got["matched_ious"]


def test_config_shape(gold, dev):
    case = "config_shape"
    c = gen.CASES[case]
    cost, iou, col4row, st_cost, st_lsa, boxes = device_costs(case, dev)
    assert not st_cost.any() and not st_lsa.any()
    for n, G in enumerate(c["G"]):
        check_valid(col4row[n], c["K"], G)
        live = cost[n, 0, :, :G]
        want = total_of(live, scipy_rows(live))                            # scipy on the device's own matrix
        assert abs(total_of(live, col4row[n]) - want) <= 1e-9 * max(1.0, abs(want)), n
    got = as_dict(get_targets(case, dev))
    want = host_mirror(case, col4row=col4row, iou=iou, boxes=boxes)        # the targets that follow from the device's own assignment
    for name in ("labels", "label_weights", "bbox_weights", "ious"):
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["bbox_targets"][..., [0, 1, 2]], want["bbox_targets"][..., [0, 1, 2]])
    assert gen.ulps(got["bbox_targets"][..., 3:8], want["bbox_targets"][..., 3:8]).max() <= 1
    assert int(got["num_pos"]) == want["num_pos"] == int(gold[case + ".num_pos"])
    assert abs(float(got["matched_ious"]) - want["matched_ious"]) <= 1.2e-7   # two fp32 roundings of a mean below 1
    assert not got["flags"].any()


def test_graph_replay_over_fresh_inputs(gold, bars, dev):
    """sync=False captured once on one fixture; every input buffer then takes another fixture with other ground-truth counts: the
    replay equals that fixture's golden with nothing left from the first."""
    first, second = "small", "small_b"
    c = gen.CASES[first]
    assert (gen.CASES[second]["K"], gen.CASES[second]["L"]) == (c["K"], c["L"])
    rows = 24
    boxes = torch.zeros((rows, 7), dtype=torch.float32, device=dev)
    labels = torch.zeros(rows, dtype=torch.int64, device=dev)
    offsets = torch.zeros(c["B"] + 1, dtype=torch.int32, device=dev)
    preds = {k: torch.zeros(v.shape, dtype=torch.float32, device=dev) for k, v in gen.inputs(first)["preds"].items()}
    coder, assigner, cfg = make_coder(first), make_assigner(first), gen.case_cfg(first)

    def load(case):
        b, l, o = (torch.from_numpy(a).to(dev) for a in gen.packed(case))
        boxes.fill_(float("nan"))                                          # rows past the live ones are never read
        boxes[:b.shape[0]].copy_(b)
        labels.fill_(-7)
        labels[:l.shape[0]].copy_(l)
        offsets.copy_(o)
        for k, v in gen.inputs(case)["preds"].items():
            preds[k].copy_(torch.from_numpy(v).to(dev))

    def step():
        return heads.transfusion_get_targets((boxes, labels, offsets), None, preds, coder, assigner, cfg, c["K"], gen.C,
                                             num_decoder_layers=c["L"], max_boxes_per_sample=9, sync=False)

    load(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                          # a capture admits no sync and no read-back
        out = step()
    for case in (first, second, first):
        load(case)
        graph.replay()
        torch.cuda.synchronize()
        got = as_dict(out)
        check_targets(case, gold, got, bars[1])
        assert not got["flags"].any()


def test_no_host_sync(dev):
    """Both input forms, second call onwards (the first builds the cached offsets of the list form): any synchronising call raises."""
    case = "layers"
    c = gen.CASES[case]
    coder, assigner, cfg = make_coder(case), make_assigner(case), gen.case_cfg(case)
    forms = [device_inputs(case, dev, form) for form in ("lists", "packed")]   # the uploads synchronise: before the guarded region

    def run():
        return [heads.transfusion_get_targets(*gt, preds, coder, assigner, cfg, c["K"], gen.C, num_decoder_layers=c["L"], sync=False, **kw)
                for preds, gt, kw in forms]

    run()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(out[0][5]) == int(out[1][5]) > 0


def test_run_to_run_bit_equality(dev):
    runs = [get_targets("config_shape", dev) for _ in range(3)]
    torch.cuda.synchronize()
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x   # noqa: E731
    assert int(runs[0][5]) > 0
    for other in runs[1:]:
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(runs[0], other))


def test_flagged_samples_are_all_negative(gold, bars, dev):
    """A sample over the bound, a non-finite logit and a label outside [0, C): that sample is all negative with its flag; the other
    sample of the batch is intact."""
    case = "small"
    c = gen.CASES[case]
    P = c["L"] * c["K"]
    preds, gt, _ = device_inputs(case, dev, "lists")

    def run(preds, gt, **kw):
        return as_dict(heads.transfusion_get_targets(*gt, preds, make_coder(case), make_assigner(case), gen.case_cfg(case), c["K"], gen.C,
                                                     num_decoder_layers=c["L"], sync=False, **kw))

    def check(got, flag):
        assert got["flags"].tolist() == [flag, 0]
        assert (got["labels"][0] == gen.C).all() and (got["label_weights"][0] == 1).all() and not got["bbox_targets"][0].any()
        assert not got["bbox_weights"][0].any() and not got["ious"][0].any()
        for name in ("labels", "label_weights", "bbox_weights"):
            assert np.array_equal(got[name][1], gold[case + "." + name][1])
        assert int(got["num_pos"]) == int((gold[case + ".bbox_weights"][1, :, 0] > 0).sum())
        assert got["labels"].shape == (c["B"], P)

    check(run(preds, gt, max_boxes_per_sample=4), head_assign.STATUS_OVERFLOW)           # 5 and 3 boxes under a bound of 4
    bad = {k: v.clone() for k, v in preds.items()}
    bad["heatmap"][0, :, 2] = float("nan")
    check(run(bad, gt), head_assign.STATUS_NONFINITE)
    labels = [l.clone() for l in gt[1]]
    labels[0][1] = gen.C
    check(run(preds, (gt[0], labels)), head_assign.STATUS_NONFINITE | head_assign.STATUS_LABEL)


def test_assigner_and_cost_classes(gold, bars, dev):
    """The reference's per-sample interface: HungarianAssigner3D.assign and the callable costs over the same kernels."""
    case = "small"
    c = gen.CASES[case]
    cost, iou, col4row, _, _, boxes = device_costs(case, dev)
    preds, gt, _ = device_inputs(case, dev, "lists")
    assigner, cfg = make_assigner(case), gen.case_cfg(case)
    for b, G in enumerate(c["G"]):
        pb = torch.from_numpy(boxes[b]).to(dev)
        res = assigner.assign(pb, gt[0][b], gt[1][b], preds["heatmap"][b:b + 1], cfg)
        want = gold[case + ".col4row"][b]
        assert res.num_gts == G and np.array_equal(res.gt_inds.cpu().numpy(), want.astype(np.int64) + 1)
        labels = np.where(want >= 0, gen.inputs(case)["gt_labels"][b][np.maximum(want, 0)], -1)
        assert np.array_equal(res.labels.cpu().numpy(), labels)
        matched = np.where(want >= 0, iou[b, 0][np.arange(c["K"]), np.maximum(want, 0)], 0).astype(np.float32)
        assert np.array_equal(res.max_overlaps.cpu().numpy(), matched)
        pair_iou = assigner.iou_calculator(pb, gt[0][b])
        total = assigner.cls_cost(preds["heatmap"][b].T, gt[1][b]) + assigner.reg_cost(pb, gt[0][b], cfg) + assigner.iou_cost(pair_iou)
        assert np.array_equal(pair_iou.cpu().numpy(), iou[b, 0, :, :G])
        assert np.abs(total.cpu().numpy() - cost[b, 0, :, :G]).max() <= 2.4e-7   # the same terms, summed by torch: one fp32 ulp below 2
    empty = assigner.assign(torch.from_numpy(boxes[0]).to(dev), gt[0][0][:0], gt[1][0][:0], preds["heatmap"][:1], cfg)
    assert empty.num_gts == 0 and empty.max_overlaps is None and not empty.gt_inds.any().item()


# ---- ha_iou3d on near-duplicate, collinear and far-away boxes against float64 (tests/iou3d_families.py) ---------------------------
@pytest.fixture(scope="module")
def lifted_refs():
    """Per family, lifted to LiDAR boxes (z = -1, height 1.5): the float64 3D IoU o h / (va + vb - o h) with o from
    oracle.rotated_overlap_float64, the same from the fp32 oracle's o, the well-conditioned mask and the device's allowance."""
    return {name: families.reference_lifted(name) for name in families.FAMILIES}


@pytest.mark.parametrize("name", families.FAMILIES)
def test_bbox_overlaps_on_family_pairs_stay_within_four_oracle_errors_of_float64(name, lifted_refs, dev):
    """The bars of test_gpu_iou3d.py's family test, through BboxOverlaps3D: pair p is the diagonal of the [P, P] result."""
    r = lifted_refs[name]
    a, b = torch.from_numpy(r["a7"]).to(dev), torch.from_numpy(r["b7"]).to(dev)
    calc = head_assign.BboxOverlaps3D()
    full = calc(a, b)
    assert torch.equal(full, calc(a, b)), f"{name}: two calls differ"
    full = full.cpu().numpy()
    got, well, allowed = np.diagonal(full).astype(np.float64), r["well"], r["bar_iou"]
    assert not np.isnan(got).any() and (got >= 0).all(), f"{name}: NaN or negative on the diagonal"
    err = np.abs(got - r["iou64"])
    worst = float(err[well].max())
    print(f"{name}: device 3D IoU max error against float64 {worst:.3g} on {int(well.sum())} well-conditioned pairs (allowed "
          f"{allowed:.3g}; oracle {r['oracle_err_iou']:.3g}); {int((err[well] > allowed).sum())} over; "
          f"{int((~well).sum())} ill-conditioned")
    record_parity(f"iou3d_family/{name}/device_iou3d_vs_f64", worst, allowed)
    assert worst <= allowed, f"{name}: {worst} > {allowed} at pair {int(np.argmax(np.where(well, err, 0)))}"
    # off the diagonal: ordinary pairs against the fp32 oracle's overlap under the same 3D formula, 1e-4
    o = oracle.iou3d_pairwise(families.lidar_bev(r["a7"]), families.lidar_bev(r["b7"]), "overlap").astype(np.float64) * 1.5
    va, vb = np.prod(r["a7"][:, 3:6].astype(np.float64), 1), np.prod(r["b7"][:, 3:6].astype(np.float64), 1)
    want = o / np.maximum(va[:, None] + vb[None, :] - o, 1e-8)
    off = ~np.eye(families.P, dtype=bool)
    assert np.max(np.abs(full[off] - want[off])) <= 1e-4


def test_bbox_overlaps_on_special_boxes_have_the_oracles_nans(dev):
    """The 16 special pairs lifted to LiDAR boxes (a zero-area box, a negative extent and so a negative volume, a NaN yaw, an inf
    coordinate, which lifts to an inf centre and size and a NaN edge, yaw = 1e4): NaN where the fp32 oracle's overlap put through
    the same 3D formula in fp32 has NaN, on all 256 entries; within 1e-4 of it on the 16 pairs where both are finite (the other
    entries pair two degenerate boxes, see test_gpu_iou3d.py); the same on a second call."""
    A, B = families.special()
    a7, b7 = families.lift(A), families.lift(B)
    a, b = torch.from_numpy(a7).to(dev), torch.from_numpy(b7).to(dev)
    calc = head_assign.BboxOverlaps3D()
    got_t = calc(a, b)
    assert torch.equal(got_t.view(torch.int32), calc(a, b).view(torch.int32)), "two calls differ"
    got = got_t.cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        o = oracle.iou3d_pairwise(families.lidar_bev(a7), families.lidar_bev(b7), "overlap") * np.float32(1.5)
        va, vb = a7[:, 3] * a7[:, 4] * a7[:, 5], b7[:, 3] * b7[:, 4] * b7[:, 5]
        want = o / np.fmax(va[:, None] + vb[None, :] - o, np.float32(1e-8))        # fmaxf: a NaN union gives the floor
    assert want.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want))
    pairs = np.isfinite(np.diagonal(got)) & np.isfinite(np.diagonal(want))
    assert pairs.sum() >= 10 and np.array_equal(np.isfinite(np.diagonal(got)), np.isfinite(np.diagonal(want)))
    assert np.max(np.abs(np.diagonal(got)[pairs] - np.diagonal(want)[pairs])) <= 1e-4
