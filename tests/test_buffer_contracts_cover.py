"""Every entry point that takes a pointer with its byte count has a guarded-buffer case in tests/test_gpu_buffer_contracts.py, or a
stated reason for having none.  Runs without a device: it reads the signature tables, the GPU module's registries and the size
functions (host code)."""
from ctypes import c_size_t, c_void_p

from bevfusion_amd import _capi

import test_gpu_buffer_contracts as gpu

MAIN = ["bev_pool_prepare", "bev_pool_prepare_from_geom", "bev_pool_fused_schedule", "bev_pool_fused_columns_count",
        "bev_pool_fused_columns_build", "sparse_bn_stats", "sparse_bn_backward", "depth_raster", "depth_raster_batch",
        "depth_raster_batch_zero_ws", "depth_inputs_batch", "depth_inputs_batch_zero_ws", "hard_voxelize", "voxelize_mean",
        "voxelize_mean_batch", "voxelize_mean_batch_ex", "voxelize_mean_batch_rows16", "spconv_hash_index_build", "spconv_downsample",
        "spconv_downsample_sorted", "spconv_build_rulebook", "spconv_pairs_from_nbr", "spconv_sorted_index_build", "spconv_conv_wgrad",
        "spconv_conv_wgrad_slab", "iou3d_nms", "exclusive_scan_u32", "exclusive_scan_u32_single_pass", "radix_sort_pairs_u32",
        "radix_sort_pairs_u32_segmented"]
EXT = ["dynamic_scatter_index", "head_proposals", "centerpoint_select", "mha_forward", "mha_backward"]

# entry points that may not be exempted
MUST_HAVE = ["exclusive_scan_u32", "exclusive_scan_u32_single_pass", "radix_sort_pairs_u32", "radix_sort_pairs_u32_segmented", "iou3d_nms",
             "bev_pool_prepare", "bev_pool_prepare_from_geom", "bev_pool_fused_schedule", "sparse_bn_stats", "sparse_bn_backward",
             "depth_raster_batch", "depth_raster_batch_zero_ws", "hard_voxelize", "voxelize_mean_batch_ex", "spconv_build_rulebook",
             "spconv_hash_index_build", "spconv_downsample", "spconv_pairs_from_nbr", "spconv_conv_wgrad", "mha_forward", "mha_backward",
             "head_proposals", "centerpoint_select"]
# entry points without scratch whose extents the headers promise
UNSIZED = ["iou3d_boxes_iou_bev", "iou3d_boxes_overlap_bev", "bev_pool_forward_cells", "bev_pool_backward_rows", "spconv_conv_forward_tiled",
           "spconv_transpose_nbr", "spconv_dense_bev", "spconv_pad_cast_rows", "sparse_bn_apply", "seg_iou_counts"]


def _sized(signatures):
    """Names (without the prefix) whose argument list has a pointer immediately followed by a size_t."""
    return sorted(name[len("bevamd_"):] for name, (_, args) in signatures.items()
                  if any(a is c_void_p and b is c_size_t for a, b in zip(args, args[1:])))


def test_the_sized_entry_points_are_the_known_ones():
    """A new entry point with a sized buffer lands here first: give it a case (or a reason) and add it to the list."""
    assert len(MAIN) == 30 and len(EXT) == 5
    assert _sized(_capi._SIGNATURES) == sorted(MAIN)
    assert _sized(_capi._EXT_SIGNATURES) == sorted(EXT)


def test_every_sized_entry_point_is_covered_or_exempt_with_a_reason():
    for name in MAIN + EXT:
        assert (name in gpu.CASES) != (name in gpu.EXEMPT), f"{name}: a case or an exemption, and not both"
    assert set(gpu.EXEMPT) <= set(MAIN + EXT) and len(gpu.EXEMPT) <= 8
    for name, reason in gpu.EXEMPT.items():
        assert name not in MUST_HAVE, f"{name} may not be exempted"
        assert isinstance(reason, str) and len(reason.strip()) > 20 and "\n" not in reason, f"{name}: one line saying why"
    for name in MUST_HAVE + UNSIZED:
        assert gpu.CASES.get(name), f"{name} has no case"
    for name, cases in gpu.CASES.items():
        assert "bevamd_" + name in _capi._SIGNATURES or "bevamd_" + name in _capi._EXT_SIGNATURES, f"{name} is no entry point"
        assert cases and all(isinstance(cid, str) and callable(run) for cid, run in cases)
        assert len({cid for cid, _ in cases}) == len(cases), f"{name}: duplicate case ids"


def test_every_covered_sized_entry_point_publishes_a_size():
    """The size functions are host code: at the tested shapes none of them answers 0 (their answer for a shape they reject), so
    check C of the GPU module (one byte short) always has a byte to withhold."""
    lib = _capi.load()
    covered = [n for n in MAIN + EXT if n in gpu.CASES]
    assert sorted(gpu.PUBLISHED) == sorted(covered)
    for name in covered:
        size = int(gpu.PUBLISHED[name](lib))
        assert size > 0, f"{name}: published size 0"
