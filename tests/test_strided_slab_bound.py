"""The bound that decides whether a strided 3x3x3 layer's filter gradient may read staged-rows metadata
(spconv/fused_train.py: strided_slab_range_bound, strided_wgrad_route) against the rulebook itself: the oracle's pairs of dense,
half-dense and sparse-output grids, the true longest range hi - lo + 1 of a 128-row output block through one kernel plane
computed in numpy.  The bound must hold everywhere, must not be loose by more than about one (y, z) plane on the dense grids, and
must keep the flagship's three strided layers on the staged-rows kernel.  No GPU."""
import numpy as np
import pytest

import oracle
from bevfusion_amd import synth
from bevfusion_amd.spconv import fused_train, ops

ROWS = 128
LIMIT = 0xFFFE


def _rows(B, shape, keep):
    """keep(b) -> bool mask over the grid's cells; rows in ascending linear index"""
    out = []
    for b in range(B):
        lin = np.flatnonzero(keep(b).reshape(-1))
        out.append(np.concatenate([np.full((len(lin), 1), b), np.stack(np.unravel_index(lin, shape), 1)], 1))
    return np.concatenate(out).astype(np.int32)


def _longest_range(indices, B, shape, padding=(1, 1, 1)):
    """max over (128-row output block, kernel plane kx) of hi - lo + 1 over the input rows the block reads through that plane"""
    oi, pairs, num, _ = oracle.get_indice_pairs(indices, B, shape, (3, 3, 3), (2, 2, 2), padding, (1, 1, 1), 0, order="cuda")
    m = oi.shape[0]
    assert np.all(np.diff(np.ravel_multi_index((indices[:, 1], indices[:, 2], indices[:, 3]), shape)
                          + indices[:, 0].astype(np.int64) * int(np.prod(shape))) > 0)
    nbr = np.full((27, m), -1, np.int64)
    for k in range(27):
        i, o = pairs[k, 0, :num[k]], pairs[k, 1, :num[k]]
        assert np.all(indices[i, 1] == 2 * oi[o, 1] - padding[0] + k // 9)         # offset k lies in kernel plane kx = k // 9
        nbr[k, o] = i
    worst = 0
    for lo_row in range(0, m, ROWS):
        for j in range(3):
            v = nbr[9 * j: 9 * j + 9, lo_row: lo_row + ROWS]
            v = v[v >= 0]
            if v.size:
                worst = max(worst, int(v.max() - v.min() + 1))
    return worst


def _planes(B, shape):
    return 2 if B > 1 and shape[0] % 2 == 0 else 1


DENSE = [(1, (7, 40, 21)), (1, (6, 64, 9)), (2, (5, 48, 11)), (2, (6, 36, 13)), (1, (3, 90, 30))]


@pytest.mark.parametrize("B,shape", DENSE)
def test_bound_holds_and_is_tight_on_dense_grids(B, shape):
    ind = _rows(B, shape, lambda b: np.ones(shape, bool))
    true = _longest_range(ind, B, shape)
    Y, Z = shape[1], shape[2]
    R = fused_train.strided_slab_range_bound(Y, Z, ROWS, _planes(B, shape))
    assert true <= R, (true, R)
    # a useless bound does not pass: the one-plane bound is the dense truth plus less than a plane (8 rows per block row, five
    # lines), and the seam term of an even X adds exactly one more
    R1 = fused_train.strided_slab_range_bound(Y, Z, ROWS, 1)
    assert true > Y * Z, "a dense block that straddles two output planes reads the plane in between"
    assert R1 - true <= 8 * ROWS + 5 * Z + Y * Z // 4, (true, R1)
    assert R - true <= Y * Z + 8 * ROWS + 5 * Z + Y * Z // 4, (true, R)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("B,shape", [(2, (9, 40, 21)), (3, (8, 30, 16)), (1, (11, 64, 9))])
def test_bound_holds_on_half_dense_and_sparse_output_grids(B, shape, seed):
    rng = np.random.default_rng(seed)
    Y, Z = shape[1], shape[2]
    R = fused_train.strided_slab_range_bound(Y, Z, ROWS, _planes(B, shape))
    half = _rows(B, shape, lambda b: rng.random(shape) < 0.5)
    assert _longest_range(half, B, shape) <= R
    # sparse outputs between filled input planes: a block runs over many output planes, the ranges keep the filled ones whole
    def sparse(b):
        keep = rng.random(shape) < 0.004
        for x in rng.choice(shape[0], size=2, replace=False):
            keep[x] = True
        return keep
    assert _longest_range(_rows(B, shape, sparse), B, shape) <= R
    # every cell of every other line: each output exists, a quarter of the inputs do
    lines = _rows(B, shape, lambda b: np.broadcast_to((np.arange(Y) % 2 == b % 2)[None, :, None], shape))
    assert _longest_range(lines, B, shape) <= R


def test_the_seam_of_an_even_grid_needs_the_second_plane():
    """Case (5) of the derivation, built: sample 0 fills its last two x-planes, sample 1 holds two cells.  The block that carries
    the last rows of sample 0 and the rows of sample 1 reads, through kx = 0, from plane X - 3 of sample 0 to plane 1 of sample 1:
    both filled planes whole — above the one-plane bound, inside the two-plane one."""
    B, shape = 2, (6, 64, 40)
    Y, Z = shape[1], shape[2]

    def keep(b):
        k = np.zeros(shape, bool)
        if b == 0:
            k[4] = k[5] = True
            k[3, 0, 0] = k[3, Y - 1, Z - 1] = True
        else:
            k[0, 0, 0] = k[1, 0, 0] = True
        return k

    true = _longest_range(_rows(B, shape, keep), B, shape)
    assert true >= 2 * Y * Z
    assert fused_train.strided_slab_range_bound(Y, Z, ROWS, 1) < true <= fused_train.strided_slab_range_bound(Y, Z, ROWS, 2)
    assert fused_train.strided_wgrad_route((6, 250, 130), 2, ROWS) == "checked"      # ... so such a grid is checked every step
    assert fused_train.strided_wgrad_route((6, 250, 130), 1, ROWS) == "staged"
    assert fused_train.strided_wgrad_route((7, 250, 130), 2, ROWS) == "staged"


def test_padding_zero_along_an_odd_z():
    """The flagship's 64 -> 128 layer pads (1, 1, 0): output oz reads cells 2 oz .. 2 oz + 2, the last output owns three."""
    B, shape, pad = 2, (7, 40, 11), (1, 1, 0)
    for keep in (lambda b: np.ones(shape, bool), lambda b: np.random.default_rng(b).random(shape) < 0.5):
        true = _longest_range(_rows(B, shape, keep), B, shape, pad)
        assert true <= fused_train.strided_slab_range_bound(shape[1], shape[2], ROWS, 1, pad_z=0)
    assert fused_train.strided_wgrad_route((7, 40, 10), 1, ROWS, (2, 2, 2), pad) == "gather"     # even Z: cells no output reads
    assert fused_train.strided_wgrad_route((7, 40, 11), 1, ROWS, (2, 2, 2), (0, 1, 1)) == "gather"
    assert fused_train.strided_wgrad_route((7, 40, 11), 1, ROWS, (2, 2, 1), (1, 1, 1)) == "gather"


def test_the_guard_keeps_the_flagship_on_the_staged_rows_kernel():
    """synth.CL_CONFIG's grid and the two below it (the inputs of 16 -> 32, 32 -> 64, 64 -> 128; the last pads (1, 1, 0)), at one
    frame and at the benchmark's batch sizes: never "gather".  Level 1 at more than one frame is the one grid whose two-plane seam
    bound exceeds the slots (2 * 1440 * 41 rows): admitted with the per-step status check."""
    shape = list(synth.CL_CONFIG["sparse_shape"])
    for pad in ((1, 1, 1), (1, 1, 1), (1, 1, 0)):
        for B in (1, 2, 4, 8):
            route = fused_train.strided_wgrad_route(shape, B, ROWS, (2, 2, 2), pad)
            assert route in ("staged", "checked"), (shape, B, route)
            assert fused_train.strided_slab_range_bound(shape[1], shape[2], ROWS, 1, pad[2]) < LIMIT
            if route == "staged":
                assert fused_train.strided_slab_range_bound(shape[1], shape[2], ROWS, _planes(B, shape), pad[2]) < LIMIT
            else:
                assert shape == list(synth.CL_CONFIG["sparse_shape"]) and B > 1
        shape = ops.get_conv_output_size(shape, [3, 3, 3], [2, 2, 2], list(pad), [1, 1, 1])
    # the dense grids of the GPU test (tests/test_gpu_train_kernels_oracle.py): more than 0xFFFE cells per x-plane
    assert fused_train.strided_wgrad_route((3, 512, 130), 1, ROWS) == "gather"
    assert fused_train.strided_wgrad_route((3, 510, 130), 1, ROWS) == "gather"
