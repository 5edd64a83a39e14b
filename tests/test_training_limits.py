"""CPU tests of the training limit (host-only calls: the layout arithmetic of hgt_layout_for, no kernel): which (out_dim, n_heads)
pairs the training path covers -- pyhgt_amd.autograd.training_supported, the one statement of the limit that hgt_conv_train's guard
calls -- and that the header declares what the wide heads need."""
import os
import re

import pytest

from pyhgt_amd import _lib
from pyhgt_amd.autograd import MAX_TRAIN_DK_PAD, logits_form, outer_form, training_supported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (out_dim, n_heads) -> padded head width
WIDE = [(256, 2, 128), (512, 4, 128), (400, 4, 128), (768, 8, 128), (1024, 8, 128), (512, 2, 256), (768, 4, 256), (256, 1, 256)]
# every layout of tests/test_backward_gpu.py, tests/test_backward_kernels_gpu.py and tools/bench_train.py
NARROW = [(64, 4), (256, 8), (200, 4), (32, 2), (16, 1), (96, 3), (128, 4), (256, 4), (400, 8), (512, 8)]
TOO_WIDE = [(512, 1), (1024, 2)]


@pytest.mark.parametrize("d,H,dkp", WIDE)
def test_wide_heads_train(d, H, dkp):
    lay = _lib.layout_for(d, H)
    assert lay.dk_pad == dkp and lay.d_pad <= 1024
    assert outer_form(dkp) == "hgt_relation_outer_wide" and logits_form(dkp) == "mfma"
    assert training_supported(d, H) == (True, "")


@pytest.mark.parametrize("d,H", NARROW)
def test_narrow_heads_still_train(d, H):
    assert _lib.layout_for(d, H).dk_pad <= 64
    assert outer_form(_lib.layout_for(d, H).dk_pad) == "hgt_relation_outer" and logits_form(_lib.layout_for(d, H).dk_pad) == "valu"
    assert training_supported(d, H) == (True, "")


@pytest.mark.parametrize("d,H", TOO_WIDE)
def test_heads_past_256_columns_are_refused_with_a_reason(d, H):
    assert _lib.layout_for(d, H).dk_pad == 512          # inference has a layout for them
    ok, reason = training_supported(d, H)
    assert ok is False
    assert "at most %d" % MAX_TRAIN_DK_PAD in reason and "out_dim=%d" % d in reason and "n_heads=%d" % H in reason and "512" in reason
    assert MAX_TRAIN_DK_PAD == 256


def test_header_declares_the_wide_entry_point_and_abi_8():
    text = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    assert re.search(r"#define HGT_ABI_VERSION 8\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+hgt_relation_outer_wide\s*\(([^)]*)\)", code)
    assert m, "include/hgt_hip.h does not declare hgt_relation_outer_wide"
    narrow = re.search(r"\bint\s+hgt_relation_outer\s*\(([^)]*)\)", code)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(m.group(1)) == norm(narrow.group(1)), "the wide entry point takes the arguments of hgt_relation_outer"
    assert _lib.SIGNATURES["hgt_relation_outer_wide"] == _lib.SIGNATURES["hgt_relation_outer"]
    lib = _lib.load()
    assert lib.hgt_abi_version() == _lib.ABI_VERSION == 8
    assert hasattr(lib, "hgt_relation_outer_wide")
