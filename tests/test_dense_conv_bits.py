"""The heads' and the trunk's dense convolutions give the bits they gave before they were folded into one kernel template
(vfa_amd/csrc/vfa_dense.h): per case of tests/dense_bits_common.py the SHA-256 of the output's contiguous float32 bytes against
tests/golden/dense_conv_bits_parent.json, recorded on the MI355X at the commit before the fold (tests/golden/make_dense_conv_bits.py).
The kernels have a fixed summation order and no float atomics, so the digests are the same on every run."""
import json

import pytest
import torch

import dense_bits_common as db
from conftest import golden_path

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

with open(golden_path("dense_conv_bits_parent.json")) as _f:
    RECORDED = json.load(_f)["cases"]


def test_every_case_is_recorded():
    assert sorted(RECORDED) == sorted(db.NAMES) and len(db.NAMES) == 14


@pytest.mark.parametrize("name", db.NAMES)
def test_bits_of_the_parent(name):
    y = db.compute(name, DEV)
    assert list(y.shape) == RECORDED[name]["shape"] and y.is_contiguous()
    got = db.digest(y)
    print(f"{name}: {got}")
    assert got == RECORDED[name]["sha256"]
