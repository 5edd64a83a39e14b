"""CPU tests of the memory-lean training mode (recompute=True): the C ABI of the counter-based dropout (csrc/hgt_dropout.hip), its
argument rules, the Python switch, and a numpy restatement of the mask rule that reproduces the published Philox4x32-10 known
answers.  The GPU side (tests/test_recompute_training_gpu.py) compares the kernels with this restatement."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import torch

import pyhgt_amd
from pyhgt_amd import _lib, HGTConv, DenseHGTConv, GNN, Classifier, Matcher
from pyhgt_amd.autograd import takes_recompute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["hgt_dropout_mask", "hgt_dropout_apply"]
INVALID = -1


# -- the mask rule, restated ---------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: counter = 4 uint32 arrays, key = 2 uint32 values -> 4 uint32 arrays."""
    M0, M1, W0, W1, LO = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85, np.uint64(0xFFFFFFFF)
    c = [np.asarray(w, dtype=np.uint64) for w in counter]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                     # 32 x 32 -> 64 bit: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def dropout_words(n, seed, offset):
    """The uint32 word of each of n elements: element i takes word i % 4 of Philox at the 64-bit counter offset + i / 4."""
    groups = (n + 3) // 4
    ctr = (np.arange(groups, dtype=np.uint64) + np.uint64(offset % 2 ** 64))          # wraps modulo 2^64 like the kernel's sum
    zero = np.zeros(groups, dtype=np.uint64)
    w = philox4x32_10([ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), zero, zero], (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)[:n]


def dropout_mask_reference(n, seed, offset, keep):
    """float32[n]: 1 / keep where the element's word < (uint32)(keep * 2^32), 0 elsewhere; keep >= 1: ones; keep <= 0: zeros."""
    keep = np.float32(keep)
    if keep >= 1:
        return np.ones(n, dtype=np.float32)
    if keep <= 0:
        return np.zeros(n, dtype=np.float32)
    thr = np.uint32(int(float(keep) * 2.0 ** 32))       # exact: a float32 times a power of two, below 2^32
    return np.where(dropout_words(n, seed, offset) < thr, np.float32(1) / keep, np.float32(0)).astype(np.float32)


def _words(text):
    return [int(t, 16) for t in text.split()]


def test_restatement_reproduces_the_published_known_answers():
    kat = [
        ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ]
    for ctr, key, out in kat:
        got = philox4x32_10([np.array([w]) for w in _words(ctr)], _words(key))
        assert [int(w[0]) for w in got] == _words(out), (ctr, key)


def test_restatement_of_the_mask_rule():
    # the first group of (seed 0, offset 0) is the all-zero known answer; word < thr decides
    w = dropout_words(6, 0, 0)
    assert [int(v) for v in w[:4]] == _words("6627e8d5 e169c58d bc57ac4c 9b00dbd8")
    m = dropout_mask_reference(4, 0, 0, 0.5)
    assert m.tolist() == [2.0, 0.0, 0.0, 0.0]                      # 0x66.. < 0x80000000 <= the others
    assert np.array_equal(dropout_mask_reference(4, 0, 0, 0.8) != 0, w[:4] < np.uint32(0xCCCCCD00))      # float32(0.8) * 2^32
    # the counter is 64 bits wide: offset 2^32 - 1 + one group carries into word 1
    a = dropout_words(8, 5, 2 ** 32 - 1)[4:]
    b = philox4x32_10([np.array([0]), np.array([1]), np.array([0]), np.array([0])], (5, 0))
    assert [int(v) for v in a] == [int(v[0]) for v in b]
    # element i of (offset) is element i - 4 of (offset + 1); the seed's high half is key word 1
    assert np.array_equal(dropout_words(12, 2 ** 63 + 9, 7)[4:], dropout_words(8, 2 ** 63 + 9, 8))
    assert not np.array_equal(dropout_words(8, 2 ** 63 + 9, 0), dropout_words(8, 9, 0))
    assert dropout_mask_reference(5, 1, 0, 1.0).tolist() == [1.0] * 5 and dropout_mask_reference(5, 1, 0, 0.0).tolist() == [0.0] * 5
    frac = float((dropout_mask_reference(1 << 16, 3, 1 << 40, 0.8) != 0).mean())
    assert abs(frac - 0.8) < 5 * (0.16 / (1 << 16)) ** 0.5


# -- the C ABI -----------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_both_prototypes_under_abi_8_and_the_binding_matches():
    text = _header()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert decl, "include/hgt_hip.h does not declare %s" % name
        params = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
        assert params == ["float* " + ("m" if name.endswith("mask") else "x"), "int64_t n", "uint64_t seed", "uint64_t offset",
                          "float keep", "void* stream"], params
        assert hasattr(lib, name), "libhgt_hip.so lacks %s" % name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_float, C.c_void_p]
    assert re.search(r"#define\s+HGT_ABI_VERSION\s+8\b", text)
    assert _lib.ABI_VERSION == 8 and _lib.load().hgt_abi_version() == 8
    assert os.path.isfile(os.path.join(ROOT, "pyhgt_amd", "csrc", "hgt_dropout.hip"))


def test_argument_rules_hold_without_a_device():
    """Host-side checks come first and n == 0 returns before any runtime call: nothing here needs a GPU (the pointer is never
    dereferenced on the host)."""
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        assert fn(p, 0, 1, 0, 0.8, None) == 0
        assert fn(p + 4, 0, 2 ** 64 - 1, 2 ** 64 - 1, 0.0, None) == 0
        assert fn(None, 16, 1, 0, 0.8, None) == INVALID
        assert fn(None, 0, 1, 0, 0.8, None) == INVALID
        assert fn(p, -1, 1, 0, 0.8, None) == INVALID
        assert fn(p, 16, 1, 0, float("nan"), None) == INVALID
        assert fn(p, 0, 1, 0, float("nan"), None) == INVALID
    assert all(v == 0.0 for v in buf)


# -- the Python switch ---------------------------------------------------------------------------------------------------------
def test_constructor_keyword_and_default():
    assert HGTConv(32, 32, 3, 4, 2).recompute is False and not takes_recompute(HGTConv(32, 32, 3, 4, 2))
    assert HGTConv(32, 32, 3, 4, 2, recompute=True).recompute is True
    assert takes_recompute(DenseHGTConv(32, 32, 3, 4, 2, recompute=True))
    assert HGTConv(32, 32, 3, 4, 2, recompute=True).last_dropout_state is None
    g = GNN(16, 32, 3, 4, 2, 2, recompute=True)
    assert takes_recompute(g) and all(takes_recompute(gc.base_conv) for gc in g.gcs)
    g = GNN(16, 32, 3, 4, 2, 2, conv_name="dense_hgt")
    assert not takes_recompute(g) and not any(takes_recompute(gc.base_conv) for gc in g.gcs)
    assert HGTConv._RUNTIME_DEFAULTS["recompute"] is False


def test_set_recompute_reaches_layers_gnn_and_heads():
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.gnn = GNN(16, 32, 3, 4, 2, 2, conv_name="hgt")
            self.dense = GNN(16, 32, 3, 4, 2, 2, conv_name="dense_hgt")
            self.cls = Classifier(32, 5)
            self.match = Matcher(32)

    m = Model()
    mods = [m.gnn, m.dense, m.cls, m.match] + [gc.base_conv for g in (m.gnn, m.dense) for gc in g.gcs]
    assert len(mods) == 8 and not any(takes_recompute(x) for x in mods)
    assert pyhgt_amd.set_recompute(m, True) is m
    assert all(takes_recompute(x) for x in mods)
    assert not any(pyhgt_amd.autograd.takes_det_route(x) for x in mods)            # the two switches are independent
    pyhgt_amd.set_recompute(m, False)
    assert not any(takes_recompute(x) for x in mods)
    assert "set_recompute" in pyhgt_amd.__all__


def test_module_unpickled_without_the_attribute_is_a_default_one():
    layer = HGTConv(32, 32, 3, 4, 2, recompute=True)
    assert pickle.loads(pickle.dumps(layer)).recompute is True          # the attribute travels with a pickle of this class
    for cls in (HGTConv, DenseHGTConv):
        st = cls(32, 32, 3, 4, 2, recompute=True).__getstate__()
        st.pop("recompute")                                             # what an earlier pickle looks like
        st.pop("last_dropout_state")
        bare = cls.__new__(cls)
        bare.__setstate__(st)
        assert bare.recompute is False and not takes_recompute(bare) and bare.last_dropout_state is None
    for mod in (GNN(16, 32, 3, 4, 2, 1, recompute=True), Classifier(32, 5), Matcher(32)):
        st = dict(mod.__dict__)
        st.pop("recompute", None)
        bare = type(mod).__new__(type(mod))
        bare.__setstate__(st)
        assert not takes_recompute(bare)


def test_state_dict_names_do_not_move():
    for cls in (HGTConv, DenseHGTConv):
        a, b = cls(32, 32, 2, 3, 4, 0.2, True, True), cls(32, 32, 2, 3, 4, 0.2, True, True, recompute=True)
        assert list(a.state_dict().keys()) == list(b.state_dict().keys()) and repr(a) == repr(b)
