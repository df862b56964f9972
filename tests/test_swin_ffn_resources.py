"""CPU: the register and scratch budget of the fused Swin FFN kernel, read from the gfx950 code object hipcc produced (see
tests/test_kernel_resources.py for the method).  DESIGN 3.30 states the occupancy the kernel is built for: a wave holds the fp32
output of 32 tokens x C channels, C / 2 registers per lane, and two waves share a SIMD at every width (at most 256 registers, VGPR
+ AGPR as the metadata counts them); no scratch and no spills in any instantiation, both storage types."""
import glob
import os
import shutil

import pytest

from test_kernel_resources import OBJ, TOOLS, _kernels

CHANNELS = [32, 64, 96, 128, 160, 192]
MAX_REGS = {c: 256 for c in CHANNELS}                             # two waves per SIMD
LDS_BYTES = {c: 32 * (c + 8) * 2 for c in CHANNELS}               # the token tile, [32][C + 8] 16-bit


@pytest.mark.skipif(not glob.glob(os.path.join(OBJ, "*.o")) or not all(os.path.exists(t) for t in TOOLS) or not shutil.which("c++filt"),
                    reason="needs the in-tree objects of bevfusion_amd.build and the ROCm llvm tools")
def test_every_instantiation_fits_its_occupancy_without_scratch():
    k = _kernels()
    found = sorted(n for n in k if "swin_ffn_kernel" in n)
    want = sorted(f"void bevamd::swin_ffn_kernel<{b}, {c}>" for b in ("false", "true") for c in CHANNELS)
    assert found == want, found
    for c in CHANNELS:
        for b in ("false", "true"):
            name = f"void bevamd::swin_ffn_kernel<{b}, {c}>"
            got = k[name]
            assert got["obj"] == "swin_ffn", got
            assert got["scratch"] == 0 and got["vgpr_spills"] == 0, (name, got)
            assert got["regs"] <= MAX_REGS[c], (name, got)
    for c in CHANNELS:                                              # the one-wave workgroups of that occupancy fit a CU's LDS
        assert LDS_BYTES[c] * 4 * (512 // MAX_REGS[c]) <= 160 * 1024, c
