"""CPU: the argument checks of the three fused 16-bit sparse-convolution forward entry points (bevamd_spconv_conv_forward_tiled,
_tiled_slots, _slab).  They run on the host before any HIP call, so every rejected argument set is driven through ctypes with
fabricated addresses that are never dereferenced.  Each case pins the return code AND the full error text, and the combined cases
pin which check fires first.  No case is a valid argument set with rows to compute: none may reach a launch."""
import pytest

from bevfusion_amd import _capi

OK, INVALID = 0, 1
FEAT, IMAGE, NBR, OUT, RES, VEC, HDR, SLOTS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000   # 16-byte aligned

_COMMON = dict(features=FEAT, dtype=1, feat_stride=32, num_in=100, image=IMAGE, num_out=100, num_out_dev=None, cin=32, cout=32,
               out=OUT, out_stride=32, bias=None, bn_scale=None, bn_shift=None, residual=None, residual_stride=0, relu=0, variant=0,
               stream=None)
_TAIL = ["out", "out_stride", "bias", "bn_scale", "bn_shift", "residual", "residual_stride", "relu", "variant", "stream"]
_HEAD = ["features", "dtype", "feat_stride", "num_in", "image"]
# entry -> (symbol, argument order, what a valid call would pass besides _COMMON)
_ENTRIES = {
    "tiled": ("bevamd_spconv_conv_forward_tiled",
              _HEAD + ["nbr", "nbr_stride", "num_out", "num_out_dev", "kernel_volume", "cin", "cout"] + _TAIL,
              dict(nbr=NBR, nbr_stride=100, kernel_volume=27)),
    "slots": ("bevamd_spconv_conv_forward_tiled_slots",
              _HEAD + ["hdr", "slots", "block_rows", "num_out", "num_out_dev", "cin", "cout"] + _TAIL,
              dict(hdr=HDR, slots=SLOTS, block_rows=128)),
    "slab": ("bevamd_spconv_conv_forward_slab",
             _HEAD + ["hdr", "slots", "block_rows", "num_out", "num_out_dev", "cin", "cout"] + _TAIL,
             dict(hdr=HDR, slots=SLOTS, block_rows=None)),     # None: what bevamd_spconv_slab_block_rows(cin, variant) says
}

G2 = 1 << 25    # rows of 32 halves (64 bytes) that make exactly 2 GiB
G4 = 1 << 26    # ... 4 GiB
PITCH_T = "feature pitch %d must be a multiple of 8 and >= %d (zero-padded), 16-byte aligned"
PITCH_S = "feature pitch %d must be a multiple of 8 and >= %d, 16-byte aligned"
BOUND_T = "feature matrix must be < 2 GiB"
BOUND_S = "the feature tensor must be smaller than 4 GiB (buffer descriptor)"
RES_S = "the residual tensor must be smaller than 4 GiB (buffer descriptor)"
BAD_OUT = dict(out_stride=31)            # fails "bad output pitch", the check behind the byte bounds


def _gather_cases(entry, own_null):
    """The checks the two gather entry points share, in their order."""
    return [
        (entry, dict(dtype=0), INVALID, "dtype 0 is not 16-bit"),
        (entry, dict(dtype=3), INVALID, "dtype 3 is not 16-bit"),
        (entry, dict(cin=0), INVALID, "bad sizes"),
        (entry, dict(cout=-1), INVALID, "bad sizes"),
        (entry, dict(num_out=-1), INVALID, "bad sizes"),
        (entry, dict(num_in=-1), INVALID, "bad sizes"),
        (entry, dict(num_out=0), OK, None),
        (entry, dict(features=None), INVALID, "null buffer"),
        (entry, dict(image=None), INVALID, "null buffer"),
        (entry, dict(out=None), INVALID, "null buffer"),
        *[(entry, {k: None}, INVALID, "null buffer") for k in own_null],
        (entry, dict(cin=129), INVALID, "channels 129 -> 32 exceed 128"),
        (entry, dict(cout=129), INVALID, "channels 32 -> 129 exceed 128"),
        (entry, dict(feat_stride=24), INVALID, PITCH_T % (24, 32)),
        (entry, dict(feat_stride=36), INVALID, PITCH_T % (36, 32)),
        (entry, dict(cin=33, feat_stride=32), INVALID, PITCH_T % (32, 64)),          # the PADDED width counts
        (entry, dict(features=FEAT + 8), INVALID, PITCH_T % (32, 32)),
        (entry, dict(num_in=G2), INVALID, BOUND_T),
        (entry, dict(num_in=G2 - 1, **BAD_OUT), INVALID, "bad output pitch"),         # one row less passes the bound
        (entry, dict(out_stride=31), INVALID, "bad output pitch"),
        (entry, dict(residual=RES, residual_stride=16), INVALID, "bad output pitch"),
        (entry, dict(bn_scale=VEC), INVALID, "scale and shift go together"),
        (entry, dict(bn_shift=VEC), INVALID, "scale and shift go together"),
        # two at once: the first in the order above fires
        (entry, dict(dtype=0, cin=0), INVALID, "dtype 0 is not 16-bit"),
        (entry, dict(num_out=-1, features=None), INVALID, "bad sizes"),
        (entry, dict(num_out=0, features=None, image=None, out=None, feat_stride=3), OK, None),   # nothing to do: nothing else is looked at
        (entry, dict(dtype=0, num_out=0), INVALID, "dtype 0 is not 16-bit"),                      # ... but dtype and sizes come first
        (entry, dict(cin=0, num_out=0), INVALID, "bad sizes"),
        (entry, dict(features=None, cin=129), INVALID, "null buffer"),
        (entry, dict(cin=129, feat_stride=24), INVALID, "channels 129 -> 32 exceed 128"),
        (entry, dict(feat_stride=24, num_in=1 << 30), INVALID, PITCH_T % (24, 32)),
        (entry, dict(num_in=G2, **BAD_OUT), INVALID, BOUND_T),
        (entry, dict(out_stride=31, bn_scale=VEC), INVALID, "bad output pitch"),
    ]


CASES = _gather_cases("tiled", ["nbr"]) + [
    ("tiled", dict(kernel_volume=0), INVALID, "bad sizes"),
    ("tiled", dict(nbr_stride=99), INVALID, "nbr_stride 99 < num_out 100"),
    ("tiled", dict(kernel_volume=0, dtype=0), INVALID, "dtype 0 is not 16-bit"),
    ("tiled", dict(kernel_volume=0, num_out=0), INVALID, "bad sizes"),
    ("tiled", dict(nbr=None, nbr_stride=99), INVALID, "null buffer"),
    ("tiled", dict(nbr_stride=99, cin=129), INVALID, "nbr_stride 99 < num_out 100"),
    ("tiled", dict(nbr_stride=99, feat_stride=24), INVALID, "nbr_stride 99 < num_out 100"),
] + _gather_cases("slots", ["hdr", "slots"]) + [
    ("slots", dict(block_rows=64), INVALID, "block_rows 64 (128 | 256)"),
    ("slots", dict(block_rows=0), INVALID, "block_rows 0 (128 | 256)"),
    ("slots", dict(block_rows=256, **BAD_OUT), INVALID, "bad output pitch"),          # 256 is accepted
    ("slots", dict(block_rows=64, cin=0), INVALID, "bad sizes"),
    ("slots", dict(block_rows=64, num_out=0), INVALID, "block_rows 64 (128 | 256)"),  # checked before the early return
    ("slots", dict(block_rows=64, hdr=None), INVALID, "block_rows 64 (128 | 256)"),
] + [
    ("slab", dict(dtype=0), INVALID, "dtype 0 is not 16-bit"),
    ("slab", dict(cin=48, cout=48), INVALID, "48 -> 48 channels"),
    ("slab", dict(cin=32, cout=64), INVALID, "32 -> 64 channels"),
    ("slab", dict(cin=0, cout=16), INVALID, "0 -> 16 channels"),
    ("slab", dict(cin=8, cout=32), INVALID, "8 -> 32 channels"),                     # 32 outputs need more than 8 inputs
    ("slab", dict(cin=256, cout=256), INVALID, "256 -> 256 channels"),
    ("slab", dict(num_out=-1), INVALID, "bad sizes"),
    ("slab", dict(num_in=-1), INVALID, "bad sizes"),
    ("slab", dict(num_out=0), OK, None),
    ("slab", dict(features=None), INVALID, "null buffer"),
    ("slab", dict(image=None), INVALID, "null buffer"),
    ("slab", dict(hdr=None), INVALID, "null buffer"),
    ("slab", dict(slots=None), INVALID, "null buffer"),
    ("slab", dict(out=None), INVALID, "null buffer"),
    ("slab", dict(block_rows=64), INVALID, "metadata built for 64-row blocks, variant 0 wants {rows}"),
    ("slab", dict(block_rows=128, variant=1999999), INVALID, "metadata built for 128-row blocks, variant 1999999 wants 0"),
    ("slab", dict(cin=5, cout=16, feat_stride=8, block_rows=128), INVALID, "metadata built for 128-row blocks, variant 0 wants 256"),
    ("slab", dict(feat_stride=24), INVALID, PITCH_S % (24, 32)),
    ("slab", dict(feat_stride=36), INVALID, PITCH_S % (36, 32)),
    ("slab", dict(cin=5, cout=16, feat_stride=0, block_rows=256), INVALID, PITCH_S % (0, 8)),     # narrow rows: padded to 8 | 16
    ("slab", dict(cin=9, cout=32, feat_stride=8, block_rows=256), INVALID, PITCH_S % (8, 16)),
    ("slab", dict(features=FEAT + 8), INVALID, PITCH_S % (32, 32)),
    ("slab", dict(num_in=G4), INVALID, BOUND_S),
    ("slab", dict(num_in=G4 - 1, **BAD_OUT), INVALID, "bad output pitch"),           # one row less passes the bound
    ("slab", dict(num_in=G2, **BAD_OUT), INVALID, "bad output pitch"),               # 2 GiB, the gather kernels' bound, is fine here
    ("slab", dict(residual=RES, residual_stride=32, num_out=G4), INVALID, RES_S),
    ("slab", dict(residual=RES, residual_stride=32, num_out=G4 - 1, **BAD_OUT), INVALID, "bad output pitch"),
    ("slab", dict(image=IMAGE + 8), INVALID, "image / slots must be 16-byte aligned"),
    ("slab", dict(slots=SLOTS + 2), INVALID, "image / slots must be 16-byte aligned"),
    ("slab", dict(out_stride=31), INVALID, "bad output pitch"),
    ("slab", dict(residual=RES, residual_stride=16), INVALID, "bad output pitch"),
    ("slab", dict(bn_scale=VEC), INVALID, "scale and shift go together"),
    ("slab", dict(bn_shift=VEC), INVALID, "scale and shift go together"),
    ("slab", dict(num_out=80_000_000), INVALID, "slot table of 4 GiB or more"),      # 27 16-bit slots a row
    # two at once
    ("slab", dict(dtype=0, cin=48, cout=48), INVALID, "dtype 0 is not 16-bit"),
    ("slab", dict(cin=48, cout=48, num_out=-1), INVALID, "48 -> 48 channels"),
    ("slab", dict(cin=48, cout=48, num_out=0), INVALID, "48 -> 48 channels"),
    ("slab", dict(num_out=0, features=None, block_rows=64, feat_stride=3), OK, None),
    ("slab", dict(num_out=-1, features=None), INVALID, "bad sizes"),
    ("slab", dict(slots=None, block_rows=64), INVALID, "null buffer"),
    ("slab", dict(block_rows=64, feat_stride=24), INVALID, "metadata built for 64-row blocks, variant 0 wants {rows}"),
    ("slab", dict(feat_stride=24, num_in=1 << 30), INVALID, PITCH_S % (24, 32)),
    ("slab", dict(num_in=G4, residual=RES, residual_stride=32, num_out=G4), INVALID, BOUND_S),
    ("slab", dict(residual=RES, residual_stride=32, num_out=G4, image=IMAGE + 8), INVALID, RES_S),
    ("slab", dict(image=IMAGE + 8, **BAD_OUT), INVALID, "image / slots must be 16-byte aligned"),
    ("slab", dict(out_stride=31, bn_scale=VEC), INVALID, "bad output pitch"),
    ("slab", dict(bn_scale=VEC, num_out=80_000_000), INVALID, "scale and shift go together"),
]


@pytest.mark.parametrize("entry,change,rc,text", CASES, ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for e, c, _, _ in CASES])
def test_forward_entry_point_rejects_before_any_launch(entry, change, rc, text):
    lib = _capi.load()
    symbol, order, own = _ENTRIES[entry]
    args = {**_COMMON, **own, **change}
    rows = lib.bevamd_spconv_slab_block_rows(32, 0)
    if args.get("block_rows", 0) is None:
        args["block_rows"] = lib.bevamd_spconv_slab_block_rows(args["cin"], args["variant"])
    # never a call that could launch: something is wrong with the arguments, or there are no rows
    assert rc == INVALID or args["num_out"] == 0
    lib.bevamd_bev_pool_forward(None, None, None, None, None, 10, 0, 1, 1, 1, 1, 1, None)     # plants another message
    assert "bev_pool" in _capi.last_error()
    got = getattr(lib, symbol)(*[args[k] for k in order])
    assert got == rc
    if rc == INVALID:
        assert _capi.last_error() == f"{symbol[len('bevamd_'):]}: {text.format(rows=rows)}"
    else:
        assert "bev_pool" in _capi.last_error()       # an accepted empty call says nothing
