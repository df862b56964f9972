"""CPU: the register and scratch budget of the shifted-window attention kernel, read from the gfx950 code object hipcc produced (see
tests/test_kernel_resources.py for the method).  DESIGN 3.29 states the occupancy the kernel is built for: four waves per SIMD,
i.e. at most 128 registers (VGPR + AGPR as the metadata counts them), no scratch and no spills; its LDS (one head's bias and four
transposed V tiles) must leave room for that many workgroups."""
import glob
import os
import shutil

import pytest

from test_kernel_resources import OBJ, TOOLS, _kernels

NAMES = ["void bevamd::window_attention_kernel<false>", "void bevamd::window_attention_kernel<true>"]
MAX_REGS = 128          # four waves per SIMD


@pytest.mark.skipif(not glob.glob(os.path.join(OBJ, "*.o")) or not all(os.path.exists(t) for t in TOOLS) or not shutil.which("c++filt"),
                    reason="needs the in-tree objects of bevfusion_amd.build and the ROCm llvm tools")
def test_both_instantiations_fit_four_waves_per_simd_without_scratch():
    k = _kernels()
    missing = [n for n in NAMES if n not in k]
    assert not missing, (missing, [n for n in k if "window_attention" in n])
    for name in NAMES:
        got = k[name]
        assert got["obj"] == "window_attention", got
        assert got["scratch"] == 0 and got["vgpr_spills"] == 0, (name, got)
        assert got["regs"] <= MAX_REGS, (name, got)
