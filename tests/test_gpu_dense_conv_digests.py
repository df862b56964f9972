"""The dense 16-bit convolution kernels (csrc/ext/dense_tile.h and the six units over it) write the bits they wrote as six
stand-alone units: tests/golden/dense_conv_digests.json was recorded from the parent of the commit that introduced the shared
header, and every case of tests/golden/make_dense_conv_digests.py is run again and its sha256 compared.  The recorder's docstring
says what the cases cover and when the file may be recorded anew (a summation order changed on purpose, never to make a
refactoring pass).
"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_dense_conv_digests", os.path.join(GOLDEN, "make_dense_conv_digests.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

CASES = recorder.cases()
with open(os.path.join(GOLDEN, "dense_conv_digests.json")) as fh:
    RECORDED = json.load(fh)


def test_the_record_holds_exactly_the_recorders_cases():
    """Every case has its digests and the file holds no others (a case renamed or dropped without recording shows here)."""
    assert {k.split("/mid")[0].split("/depth")[0].split("/ctx")[0] for k in RECORDED} == set(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_equal_the_recorded_ones(dev, name):
    with torch.no_grad():
        got = {name + suffix: recorder.digest(t) for suffix, t in CASES[name](dev).items()}
    assert got == {k: RECORDED[k] for k in got}
