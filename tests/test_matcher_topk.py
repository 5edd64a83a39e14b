"""Matcher retrieval, the parts that need no GPU: the numpy rules (np_matcher_scores / np_matcher_topk / np_matcher_rank) against a
brute-force sort with the tie rule -- rows full of ties, +-inf, -0 / +0, NaN, k > N, N == 0 --, against the reference's Matcher in
float64 where the reference tree is present, and the boundary: header, bindings and Makefile list the new file and symbols,
HGT_TOPK_MAX_K is mirrored and the ABI is still 8."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import pyhgt_amd
from oracle.reference_loader import reference_available, load_reference_model
from pyhgt_amd import _lib
from pyhgt_amd.metrics import matcher_scale, np_matcher_rank, np_matcher_scores, np_matcher_topk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_order(col):
    """positions of one query's scores, best first, by pairwise comparison: floats compare as floats (-0 == +0), every NaN is one
    value above +inf, equal scores go by position"""
    def before(a, b):
        sa, sb = float(col[a]), float(col[b])
        na, nb = math.isnan(sa), math.isnan(sb)
        if na != nb:
            return -1 if na else 1
        if not na and sa != sb:
            return -1 if sa > sb else 1
        return -1 if a < b else (1 if a > b else 0)
    return sorted(range(len(col)), key=functools.cmp_to_key(before))


def brute_topk(s, k):
    N, Q = s.shape
    values = np.full((Q, k), -np.inf, np.float32)
    indices = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        order = brute_order(s[:, q])[:k]
        values[q, :len(order)] = s[order, q]
        indices[q, :len(order)] = order
    return values, indices


def same_values(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def special_rows(rng, N, Q, d):
    """tx, ty whose scores hold thousands of ties, +-inf, NaN (inf * 0) and -0 / +0"""
    tx = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    ty = rng.integers(-2, 3, size=(Q, d)).astype(np.float32)
    if N >= 8:
        tx[1] = 0.0
        tx[1, 0] = np.inf                                # +inf, -inf or NaN against every query, by the sign of ty[:, 0]
        tx[3] = 0.0
        tx[3, 0] = -np.inf
        tx[5] = -0.0                                     # -0 products: must tie with the +0 rows
        tx[6] = 0.0
    if N >= 8 and Q >= 3:
        ty[:3, 0] = (0.0, 2.0, -1.0)                     # NaN, (+inf, -inf) and (-inf, +inf) from rows 1 and 3
    return tx, ty


@pytest.mark.parametrize("N,Q,d,k", [(0, 3, 8, 4), (1, 2, 4, 1), (1, 2, 4, 5), (40, 5, 8, 1), (40, 5, 8, 7), (40, 5, 8, 40), (40, 5, 8, 64),
                                     (300, 4, 16, 10), (300, 0, 16, 10)])
def test_rules_equal_a_brute_force_sort_with_the_tie_rule(N, Q, d, k):
    rng = np.random.default_rng(100 * N + 10 * Q + k)
    tx, ty = special_rows(rng, N, Q, d)
    scale = matcher_scale(d)
    s = np_matcher_scores(tx, ty, scale)
    assert s.shape == (N, Q) and s.dtype == np.float32
    if N >= 8 and Q:
        assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any()
        assert max(np.unique(s[:, q], return_counts=True)[1].max() for q in range(Q)) > 3              # ties
    values, indices = np_matcher_topk(tx, ty, k, scale)
    bv, bi = brute_topk(s, k)
    assert values.dtype == np.float32 and indices.dtype == np.int64 and values.shape == (Q, k)
    assert np.array_equal(indices, bi) and same_values(values, bv)
    assert np.all(indices[:, min(k, N):] == -1) and np.all(np.isneginf(values[:, min(k, N):]))
    index = rng.integers(-2, N + 2, size=Q)
    rank = np_matcher_rank(tx, ty, index, scale)
    assert rank.dtype == np.int64
    for q in range(Q):
        want = brute_order(s[:, q]).index(index[q]) if 0 <= index[q] < N else -1
        assert rank[q] == want
    for j in range(min(k, N)):                                                                          # rank of the j-th answer is j
        assert np.array_equal(np_matcher_rank(tx, ty, indices[:, j], scale), np.full(Q, j))


def test_zero_signs_tie_and_nan_stands_above_inf():
    tx = np.zeros((8, 4), np.float32)
    tx[:, 0] = (0.0, -0.0, np.nan, np.inf, 1.0, np.nan, -np.inf, np.inf)
    ty = np.array([[1.0, 0, 0, 0]], np.float32)
    values, indices = np_matcher_topk(tx, ty, 8, np.float32(1.0))
    assert indices.tolist() == [[2, 5, 3, 7, 4, 0, 1, 6]]
    assert np.isnan(values[0, :2]).all() and values[0, 2:].tolist() == [np.inf, np.inf, 1.0, 0.0, 0.0, -np.inf]
    assert not np.signbit(values[0, 5:7]).any()                                     # a -0 is returned as +0
    assert np_matcher_rank(tx, ty, [1], np.float32(1.0)).tolist() == [6]
    assert np_matcher_rank(tx, ty, [8], np.float32(1.0)).tolist() == [-1] and np_matcher_rank(tx, ty, [-1], np.float32(1.0)).tolist() == [-1]


def test_scale_is_the_float32_nearest_to_the_inverse_root_and_applied_once():
    for n_hid in (4, 64, 100, 256, 400, 1024):
        assert matcher_scale(n_hid).dtype == np.float32 and matcher_scale(n_hid) == np.float32(1.0 / math.sqrt(n_hid))
    tx = np.array([[3, 1, 0, 2]], np.float32)
    ty = np.array([[1, 1, 5, 2]], np.float32)
    assert np_matcher_scores(tx, ty, np.float32(0.3))[0, 0] == np.float32(8.0) * np.float32(0.3)
    with pytest.raises(ValueError):
        np_matcher_topk(tx, ty, 0, 1.0)
    with pytest.raises(ValueError):
        np_matcher_scores(tx, ty[:, :3], 1.0)
    with pytest.raises(ValueError):
        np_matcher_rank(tx, ty, [0, 0], 1.0)


@pytest.mark.skipif(not reference_available(), reason="the reference tree is not present")
def test_rules_equal_the_reference_matcher_in_float64():
    ref = load_reference_model()
    torch.manual_seed(5)
    n_hid, N, Q, k = 16, 200, 7, 10
    m = ref.Matcher(n_hid).double()
    x, y = torch.randn(N, n_hid, dtype=torch.float64), torch.randn(Q, n_hid, dtype=torch.float64)
    with torch.no_grad():
        dense = m(x, y).numpy()                                                    # [N, Q]: matmul(tx, ty^T) / sqrt(n_hid)
        tx = m.left_linear(x).float().numpy()
        ty = m.right_linear(y).float().numpy()
    scale = matcher_scale(n_hid)
    s = np_matcher_scores(tx, ty, scale)
    # float32 inputs of a float64 product and one float32 rounding each for the sum and the scale: a few ulp of the largest term
    bound = 8 * 2.0 ** -24 * (np.abs(tx) @ np.abs(ty).T) * float(scale) + 1e-30
    assert np.all(np.abs(s - dense) <= bound)
    values, indices = np_matcher_topk(tx, ty, k, scale)
    rank = np_matcher_rank(tx, ty, indices[:, 3], scale)
    assert np.array_equal(rank, np.full(Q, 3))
    for q in range(Q):
        order = np.argsort(-dense[:, q], kind="stable")                            # the reference's scores, top-k by a stable sort
        gap = np.abs(np.diff(dense[order[:k + 1], q])).min()
        order = order[:k]
        if gap > 2 * bound[:, q].max():                                            # (an order float32 rounding cannot change)
            assert np.array_equal(indices[q], order)
        assert np.all(np.abs(values[q] - dense[order, q]) <= 2 * bound[:, q].max())


NEW_SYMBOLS = ("hgt_matcher_topk_bytes", "hgt_matcher_topk", "hgt_matcher_rank")


def test_header_bindings_and_makefile_list_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    assert re.search(r"#define HGT_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    assert int(re.search(r"#define HGT_TOPK_MAX_K (\d+)", header).group(1)) == _lib.TOPK_MAX_K >= 128
    for name in NEW_SYMBOLS:
        decl = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    makefile = open(os.path.join(ROOT, "pyhgt_amd", "csrc", "Makefile")).read()
    assert "hgt_matcher_topk.hip" in makefile and os.path.isfile(os.path.join(ROOT, "pyhgt_amd", "csrc", "hgt_matcher_topk.hip"))
    lib = _lib.load()
    assert lib.hgt_abi_version() == 8 and all(hasattr(lib, name) for name in NEW_SYMBOLS)
    for name in ("np_matcher_scores", "np_matcher_topk", "np_matcher_rank", "matcher_topk", "matcher_rank", "matcher_scale"):
        assert name in pyhgt_amd.__dict__, name
    assert callable(pyhgt_amd.Matcher.topk) and callable(pyhgt_amd.Matcher.rank_of)
    check = open(os.path.join(ROOT, "tools", "matcher_topk_abi_check.cpp")).read()
    assert "-fsanitize=address,undefined" in check and "int main()" in check and all(name in check for name in NEW_SYMBOLS)


def test_scratch_size_is_host_arithmetic_and_refuses_what_the_header_says():
    import ctypes as C
    lib = _lib.load()
    nb = C.c_uint64()
    assert lib.hgt_matcher_topk_bytes(1 << 20, 256, 100, 0, C.byref(nb)) == 0
    default = nb.value
    assert 0 < default < (1 << 20) * 256 * 4 // 8                                   # far below the dense matrix
    assert lib.hgt_matcher_topk_bytes(1 << 22, 256, 100, 0, C.byref(nb)) == 0 and nb.value == default      # ... and independent of N
    assert lib.hgt_matcher_topk_bytes(5000, 64, 10, 128, C.byref(nb)) == 0 and nb.value >= 40 * 64 * 10 * 8
    assert lib.hgt_matcher_topk_bytes(5000, 64, 0, 0, C.byref(nb)) == -1
    assert lib.hgt_matcher_topk_bytes(-1, 64, 10, 0, C.byref(nb)) == -1
    assert lib.hgt_matcher_topk_bytes(5000, 64, 10, 0, None) == -1
    assert lib.hgt_matcher_topk_bytes(5000, 64, _lib.TOPK_MAX_K + 1, 0, C.byref(nb)) == -2
    assert lib.hgt_matcher_topk_bytes(5000, 2 ** 31 - 1, 10, 0, C.byref(nb)) == -2
    assert lib.hgt_matcher_topk_bytes(2 ** 31 - 1, 64, 10, 0, C.byref(nb)) == -4


def test_cpu_tensors_are_refused_like_the_other_heads():
    m = pyhgt_amd.Matcher(8)
    with pytest.raises(RuntimeError, match="np_matcher_topk"):
        m.topk(torch.zeros(5, 8), torch.zeros(2, 8), 3)
    with pytest.raises(RuntimeError, match="np_matcher_rank"):
        m.rank_of(torch.zeros(5, 8), torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="np_matcher_topk"):
        pyhgt_amd.matcher_topk(torch.zeros(5, 8), torch.zeros(2, 8), 3, 1.0)
    assert m.cache is None
