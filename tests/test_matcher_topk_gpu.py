"""Matcher retrieval on the GPU (csrc/hgt_matcher_topk.hip) against the numpy rules of pyhgt_amd.metrics.

Exact cases: small integers in [-4, 4], for which every fp32 product and sum is exact in any order, so values and indices must equal
np_matcher_topk bit for bit -- thousands of ties included -- and the ranks np_matcher_rank, for chunk_rows = 0 (the library's choice),
one step (128 rows) and a ragged last chunk.  Random floats are held to the fp32 accumulation bound
tol(c, q) = gamma_d * sum_i |tx_ci ty_qi| * scale, gamma_d = d 2^-24 / (1 - d 2^-24), against float64."""
import ctypes as C
import importlib.util
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import pyhgt_amd
from pyhgt_amd import _lib
from pyhgt_amd.metrics import matcher_rank, matcher_scale, matcher_topk, np_matcher_rank, np_matcher_scores, np_matcher_topk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
MAX_K = _lib.TOPK_MAX_K
CHUNKS = (0, 128, 384)            # the library's choice; one step of a workgroup; 3 steps: a ragged last chunk unless 384 divides N


@pytest.fixture(autouse=True, scope="module")
def leave_the_process_as_found():
    """Other files hold memory tests that count whole allocator blocks (tests/test_recompute_training_gpu.py), and which cached block
    a tensor of theirs lands in depends on every allocation made in the process before.  So this file allocates from a memory pool of
    its own -- the default pool's blocks are neither used, split nor released by it (hence no empty_cache() below) --, puts the plan
    cache back as it found it (the example's forwards would evict, and so free, the plans of earlier files), and restores the random
    generators it seeds."""
    from pyhgt_amd import GraphPlan
    with GraphPlan._cache_lock:
        kept = OrderedDict(GraphPlan._cache)
    rng_host, rng_dev = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
    with GraphPlan._cache_lock:
        GraphPlan._cache.clear()
        GraphPlan._cache.update(kept)
    torch.set_rng_state(rng_host)
    torch.cuda.set_rng_state(rng_dev, DEV)
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    """equal float arrays: NaN in the same places, the same value elsewhere (-0 == +0: the rule returns +0 for both)"""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def integer_rows(N, Q, d, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, size=(N, d)).astype(np.float32), rng.integers(-4, 5, size=(Q, d)).astype(np.float32)


def check_exact(tx, ty, k, scale, tx_dev=None, ty_dev=None):
    tx_dev = dev(tx) if tx_dev is None else tx_dev
    ty_dev = dev(ty) if ty_dev is None else ty_dev
    N, Q = tx.shape[0], ty.shape[0]
    want_v, want_i = np_matcher_topk(tx, ty, k, scale)
    rng = np.random.default_rng(N + 7 * Q + k)
    index = rng.integers(-2, N + 2, size=Q)                      # indices outside [0, N) among them
    if Q:
        index[0] = N
    want_r = np_matcher_rank(tx, ty, index, scale)
    first = None
    for rows in CHUNKS:
        v, i = matcher_topk(tx_dev, ty_dev, k, scale, chunk_rows=rows)
        r = matcher_rank(tx_dev, ty_dev, dev(index), scale, chunk_rows=rows)
        assert v.dtype == torch.float32 and i.dtype == torch.int64 and r.dtype == torch.int64
        assert tuple(v.shape) == (Q, k) and tuple(i.shape) == (Q, k) and tuple(r.shape) == (Q,)
        v, i, r = v.cpu().numpy(), i.cpu().numpy(), r.cpu().numpy()
        assert np.array_equal(i, want_i), "indices, chunk_rows=%d" % rows
        assert same_bits(v, want_v), "values, chunk_rows=%d" % rows
        assert np.array_equal(r, want_r), "ranks, chunk_rows=%d" % rows
        if first is None:
            first = v
        assert np.array_equal(v.view(np.int32), first.view(np.int32)), "the bits depend on chunk_rows"


# every N, Q, d and k of the lists below appears; k > N, N == 0, Q == 0, sizes on both sides of the 32-row tile, the 128-row step, the
# 32 / 64-query block and the three list capacities (k <= 32, <= 64, <= 128)
#   N in {0, 1, 31, 32, 33, 255, 256, 257, 1000, 4099}   Q in {0, 1, 3, 33, 64, 65}   d in {4, 64, 100, 256, 400, 1024}
#   k in {1, 2, 10, 128, MAX_K}
EXACT_CASES = [
    (0, 3, 64, 10), (0, 65, 4, MAX_K), (1, 1, 4, 1), (1, 3, 100, 2), (31, 33, 64, 10), (31, 1, 1024, MAX_K), (32, 64, 256, 2),
    (32, 3, 4, 128), (33, 65, 100, 10), (33, 0, 64, 1), (255, 1, 400, 128), (255, 64, 64, 1), (256, 33, 4, 10), (256, 65, 1024, 2),
    (257, 3, 256, MAX_K), (257, 64, 100, 10), (1000, 65, 400, 10), (1000, 33, 64, 128), (1000, 1, 256, 1), (4099, 64, 64, 10),
    (4099, 3, 1024, 2), (4099, 65, 100, MAX_K), (4099, 33, 256, 40), (4099, 1, 4, 64), (1000, 0, 400, 2),
]


@pytest.mark.parametrize("N,Q,d,k", EXACT_CASES)
def test_integer_inputs_equal_the_rule_bit_for_bit_for_every_chunking(N, Q, d, k):
    tx, ty = integer_rows(N, Q, d, seed=N * 131 + Q * 17 + d + k)
    check_exact(tx, ty, k, matcher_scale(d))


@pytest.mark.parametrize("pad_x,pad_y,shift", [(4, 8, 0), (3, 1, 0), (0, 0, 1)])
def test_strided_and_unaligned_rows(pad_x, pad_y, shift):
    """rows inside wider tensors (ld > d): 16-byte aligned rows, rows that are not (ld % 4 != 0), and a base 4 bytes off"""
    N, Q, d, k = 777, 37, 100, 10
    tx, ty = integer_rows(N, Q, d, seed=5)
    wide_x = torch.full((N, shift + d + pad_x), 1e30, dtype=torch.float32, device=DEV)
    wide_y = torch.full((Q, shift + d + pad_y), -1e30, dtype=torch.float32, device=DEV)
    wide_x[:, shift:shift + d] = dev(tx)
    wide_y[:, shift:shift + d] = dev(ty)
    xs, ys = wide_x[:, shift:shift + d], wide_y[:, shift:shift + d]
    assert xs.stride(0) == shift + d + pad_x and (pad_x + shift == 0 or not xs.is_contiguous())
    check_exact(tx, ty, k, matcher_scale(d), xs, ys)


def test_two_hundred_thousand_candidates():
    N, Q, d, k = 200000, 64, 64, 10
    tx, ty = integer_rows(N, Q, d, seed=11)
    scale = matcher_scale(d)
    want_v, want_i = np_matcher_topk(tx, ty, k, scale)
    index = np.random.default_rng(12).integers(0, N, size=Q)
    index[:4] = (-1, N, 0, N - 1)
    want_r = np_matcher_rank(tx, ty, index, scale)
    tx_dev, ty_dev = dev(tx), dev(ty)
    for rows in (0, 128, 4992):
        v, i = matcher_topk(tx_dev, ty_dev, k, scale, chunk_rows=rows)
        r = matcher_rank(tx_dev, ty_dev, dev(index), scale, chunk_rows=rows)
        assert np.array_equal(i.cpu().numpy(), want_i) and same_bits(v.cpu().numpy(), want_v), rows
        assert np.array_equal(r.cpu().numpy(), want_r), rows


# ---------------------------------------------------------------------------------------------- a score is a function of its two rows
def all_scores(tx_dev, ty_dev, scale):
    """[Q, N] int32 bit patterns of every score, read back through top-k with k = N <= MAX_K"""
    N = tx_dev.size(0)
    v, i = matcher_topk(tx_dev, ty_dev, N, scale)
    out = torch.empty_like(v)
    out.scatter_(1, i, v)
    return out.cpu().numpy().view(np.int32)


def test_scores_are_a_function_of_the_two_rows():
    rng = np.random.default_rng(21)
    N, Q, d = 90, 45, 100
    tx, ty = rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((Q, d)).astype(np.float32)
    scale = matcher_scale(d)
    base = all_scores(dev(tx), dev(ty), scale)
    pc, pq = rng.permutation(N), rng.permutation(Q)
    perm = all_scores(dev(tx[pc]), dev(ty[pq]), scale)
    assert np.array_equal(perm, base[pq][:, pc])                                  # permuting rows permutes the bits
    extra = rng.standard_normal((37, d)).astype(np.float32)
    more = all_scores(dev(np.concatenate([extra, tx])), dev(ty), scale)
    assert np.array_equal(more[:, 37:], base)                                     # prepended rows leave the old rows' bits alone
    fewer = all_scores(dev(tx), dev(ty[:1]), scale)
    assert np.array_equal(fewer, base[:1])                                        # ... and so does another number of queries


def test_top_values_follow_a_permutation_of_many_candidates():
    rng = np.random.default_rng(22)
    N, Q, d, k = 3000, 33, 256, MAX_K
    tx, ty = rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((Q, d)).astype(np.float32)
    scale = matcher_scale(d)
    v0, i0 = matcher_topk(dev(tx), dev(ty), k, scale)
    pc, pq = rng.permutation(N), rng.permutation(Q)
    v1, i1 = matcher_topk(dev(tx[pc]), dev(ty[pq]), k, scale, chunk_rows=256)
    v0, i0, v1, i1 = (t.cpu().numpy() for t in (v0, i0, v1, i1))
    assert np.array_equal(v1.view(np.int32), v0[pq].view(np.int32))
    if all(np.unique(row).size == k for row in v0):                               # (no ties: the answers are the same candidates)
        assert np.array_equal(pc[i1], i0[pq])


def test_rank_of_the_j_th_answer_is_j():
    rng = np.random.default_rng(23)
    N, Q, d, k = 3000, 33, 64, 24
    tx = rng.standard_normal((N, d)).astype(np.float32)
    tx[100:140] = tx[50]                                                          # equal rows: ties among the best
    ty = rng.standard_normal((Q, d)).astype(np.float32)
    tx_dev, ty_dev, scale = dev(tx), dev(ty), matcher_scale(d)
    v, i = matcher_topk(tx_dev, ty_dev, k, scale, chunk_rows=128)
    want = torch.arange(k, device=DEV).expand(Q, k)
    got = torch.stack([matcher_rank(tx_dev, ty_dev, i[:, j], scale) for j in range(k)], dim=1)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- random floats against float64
@pytest.mark.parametrize("N,Q,d,k", [(257, 3, 4, 10), (1000, 65, 100, 10), (4099, 33, 256, MAX_K), (2000, 64, 400, 2), (1500, 1, 1024, 40)])
def test_random_floats_against_float64(N, Q, d, k):
    rng = np.random.default_rng(N + d)
    tx, ty = rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((Q, d)).astype(np.float32)
    scale = matcher_scale(d)
    s64 = (tx.astype(np.float64) @ ty.astype(np.float64).T) * float(scale)                          # [N, Q]
    gamma = d * 2.0 ** -24 / (1 - d * 2.0 ** -24)
    tol = gamma * (np.abs(tx).astype(np.float64) @ np.abs(ty).astype(np.float64).T) * float(scale)  # [N, Q]: not a measured number
    tx_dev, ty_dev = dev(tx), dev(ty)
    v, i = (t.cpu().numpy() for t in matcher_topk(tx_dev, ty_dev, k, scale))
    m = min(k, N)
    index = rng.integers(0, N, size=Q)
    r = matcher_rank(tx_dev, ty_dev, dev(index), scale).cpu().numpy()
    for q in range(Q):
        iq, vq = i[q, :m], v[q, :m].astype(np.float64)
        assert np.unique(iq).size == m and iq.min() >= 0 and iq.max() < N
        err = np.abs(vq - s64[iq, q])
        print("N=%d d=%d q=%d: max |value - float64| / tol = %.3f" % (N, d, q, (err / tol[iq, q]).max()))
        assert np.all(err <= tol[iq, q])                                          # every value within tol of float64 at its index
        assert np.all(np.diff(v[q, :m]) <= 0)                                     # non-increasing
        ties = np.diff(v[q, :m]) == 0
        assert np.all(np.diff(iq)[ties] > 0)                                      # ties index-ascending
        rest = np.ones(N, bool)
        rest[iq] = False
        if rest.any():                                                            # nothing left out beats the k-th by more than the tolerances
            last = iq[-1]
            assert np.all(s64[rest, q] - s64[last, q] <= tol[rest, q] + tol[last, q])
        t = index[q]
        lo = np.sum(s64[:, q] - tol[:, q] > s64[t, q] + tol[t, q])
        hi = np.sum(s64[:, q] + tol[:, q] >= s64[t, q] - tol[t, q])
        assert lo <= r[q] <= hi


# ---------------------------------------------------------------------------------------------- NaN and infinities
def test_nan_stands_above_inf_and_infinities_are_placed():
    N, Q, d, k = 500, 40, 64, 30
    tx, ty = integer_rows(N, Q, d, seed=31)
    ty[:, 0] = np.resize(np.array([0.0, 2.0, -1.0], np.float32), Q)               # inf * 0 = NaN, +inf, -inf by query
    for row, val in ((7, np.inf), (400, np.inf), (13, -np.inf), (300, -np.inf), (499, np.inf)):
        tx[row] = 0.0
        tx[row, 0] = val
    tx[20] = -0.0
    tx[21] = 0.0
    s = np_matcher_scores(tx, ty, matcher_scale(d))
    assert np.isnan(s[:, 0]).sum() == 5 and np.isposinf(s[:, 1]).sum() == 3 and np.isneginf(s[:, 1]).sum() == 2
    check_exact(tx, ty, k, matcher_scale(d))
    v, i = matcher_topk(dev(tx), dev(ty), k, matcher_scale(d))
    assert i[0, :5].tolist() == [7, 13, 300, 400, 499] and bool(torch.isnan(v[0, :5]).all())       # NaN first, ties to the lower position
    assert i[1, :3].tolist() == [7, 400, 499] and bool(torch.isposinf(v[1, :3]).all())
    assert i[2, :2].tolist() == [13, 300]
    check_exact(tx, ty, MAX_K, matcher_scale(d))


# ---------------------------------------------------------------------------------------------- through Matcher
def test_matcher_methods_use_the_cache_and_equal_the_dense_scores():
    torch.manual_seed(41)
    n_hid, N, Q, k = 64, 3000, 33, 10
    m = pyhgt_amd.Matcher(n_hid).to(DEV).eval()
    x, y = torch.randn(N, n_hid, device=DEV), torch.randn(Q, n_hid, device=DEV)
    assert m.cache is None
    v, i = m.topk(x, y, k, infer=True)
    cache = m.cache
    assert cache is not None and tuple(cache.shape) == (N, n_hid)
    v2, i2 = m.topk(torch.zeros_like(x), y, k, infer=True)                       # the cache is used, as in forward: x is not read
    assert m.cache is cache and torch.equal(i, i2) and torch.equal(v, v2)
    r = m.rank_of(x, y, i[:, 3], infer=True)
    assert m.cache is cache and r.tolist() == [3] * Q
    v3, i3 = m.topk(x, y, k)                                                      # without infer: projected again, the cache stays
    assert m.cache is cache and torch.equal(i, i3) and torch.equal(v, v3)
    assert not v.requires_grad and not r.requires_grad
    with torch.no_grad():
        dense = m(x, y, infer=True)                                               # [N, Q], the existing path
        tx = cache.cpu().numpy()
        ty = torch.nn.functional.linear(y, m.right_linear.weight, m.right_linear.bias).cpu().numpy()
    assert m.cache is cache and tuple(dense.shape) == (N, Q)
    dense = dense.cpu().numpy().astype(np.float64)
    # both paths are fp32 dot products of the same projected rows, each within tol of the float64 product: 2 tol between them; forward
    # also rounds ty / sqrt(n_hid) once per element, which moves its score by at most 2^-24 * sum |tx ty| * scale < tol / d.  So a
    # value and the dense score at its index differ by at most (2 + 1 / d) tol, and where this path puts c before c' the dense scores
    # can stand the other way round by at most (2 + 1 / d) (tol_c + tol_c')
    gamma = n_hid * 2.0 ** -24 / (1 - n_hid * 2.0 ** -24)
    tol = gamma * (np.abs(tx).astype(np.float64) @ np.abs(ty).astype(np.float64).T) * float(matcher_scale(n_hid))
    both = 2.0 + 1.0 / n_hid
    v, i = v.cpu().numpy().astype(np.float64), i.cpu().numpy()
    for q in range(Q):
        gap = np.abs(v[q] - dense[i[q], q]) / tol[i[q], q]
        print("q=%d: max |topk value - dense score| / tol = %.3f" % (q, gap.max()))
        assert np.all(gap <= both)
        rest = np.ones(N, bool)
        rest[i[q]] = False
        assert np.all(dense[rest, q] - dense[i[q, -1], q] <= both * (tol[rest, q] + tol[i[q, -1], q]))
        assert np.all(np.diff(dense[i[q], q]) <= both * (tol[i[q, 1:], q] + tol[i[q, :-1], q]))          # the order is the dense scores' order


def test_peak_memory_stays_below_the_dense_matrix():
    n_hid, N, Q, k = 32, 262144, 64, 10
    m = pyhgt_amd.Matcher(n_hid).to(DEV).eval()
    x, y = torch.randn(N, n_hid, device=DEV), torch.randn(Q, n_hid, device=DEV)
    target = torch.randint(0, N, (Q,), device=DEV)
    m.topk(x[:256], y, k)                                                         # (loads the library and its kernels)
    torch.cuda.synchronize()
    dense_bytes = N * Q * 4                                                       # 64 MiB: not forming it is the feature
    for call in (lambda: m.topk(x, y, k), lambda: m.rank_of(x, y, target)):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        print("peak allocation of the call: %.1f MiB (dense matrix: %.1f MiB)" % (peak / 2 ** 20, dense_bytes / 2 ** 20))
        assert peak < dense_bytes
        del out
    v, i = m.topk(x, y, k)
    assert m.rank_of(x, y, i[:, 0]).tolist() == [0] * Q


# ---------------------------------------------------------------------------------------------- refusals and edges
def test_refusals_raise_the_documented_error_without_a_launch():
    x, y = torch.zeros(50, 64, device=DEV), torch.zeros(5, 64, device=DEV)
    with pytest.raises(RuntimeError, match=r"code -2"):
        matcher_topk(x, y, MAX_K + 1, 0.125)
    with pytest.raises(ValueError):
        matcher_topk(x, y, 0, 0.125)
    with pytest.raises(RuntimeError, match=r"code -1"):
        matcher_topk(x, y, 3, float("nan"))
    with pytest.raises(RuntimeError, match=r"code -1"):
        matcher_rank(x, y, torch.zeros(5, dtype=torch.int64, device=DEV), float("inf"))
    with pytest.raises(RuntimeError, match=r"code -2"):
        matcher_topk(x[:, :6], y[:, :6], 3, 0.125)                                # d % 4
    with pytest.raises(RuntimeError, match=r"code -2"):
        matcher_topk(torch.zeros(8, 1028, device=DEV), torch.zeros(2, 1028, device=DEV), 3, 0.125)
    with pytest.raises(RuntimeError, match=r"code -1"):
        matcher_topk(x, y, 3, 0.125, chunk_rows=-1)
    with pytest.raises(ValueError):
        matcher_rank(x, y, torch.zeros(4, dtype=torch.int64, device=DEV), 0.125)
    with pytest.raises(ValueError):
        matcher_topk(x, y[:, :32], 3, 0.125)
    with pytest.raises(TypeError):
        matcher_topk(x.double(), y.double(), 3, 0.125)
    with pytest.raises(RuntimeError, match="np_matcher_topk"):
        matcher_topk(x.cpu(), y.cpu(), 3, 0.125)
    m = pyhgt_amd.Matcher(64).to(DEV)
    with pytest.raises(RuntimeError, match="np_matcher_rank"):
        m.rank_of(x.cpu(), y, torch.zeros(5, dtype=torch.int64))
    # the entry points themselves, with device memory behind every pointer: a leading dimension below d, missing outputs, short scratch
    lib = _lib.load()
    nb = C.c_uint64()
    assert lib.hgt_matcher_topk_bytes(50, 5, 3, 0, C.byref(nb)) == 0
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=DEV)
    val, idx = torch.full((5, 3), 7.0, device=DEV), torch.full((5, 3), 7, dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda ldx, ldy, v, i, w, nbytes: lib.hgt_matcher_topk(x.data_ptr(), ldx, 50, y.data_ptr(), ldy, 5, 64, 0.125, 3, 0, v, i, w, nbytes, st)
    assert call(63, 64, val.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel()) == -1
    assert call(64, 60, val.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel()) == -1
    assert call(64, 64, None, idx.data_ptr(), ws.data_ptr(), ws.numel()) == -1
    assert call(64, 64, val.data_ptr(), None, ws.data_ptr(), ws.numel()) == -1
    assert call(64, 64, val.data_ptr(), idx.data_ptr(), None, ws.numel()) == -3
    assert call(64, 64, val.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel() - 1) == -3
    torch.cuda.synchronize()
    assert bool((val == 7.0).all()) and bool((idx == 7).all())                    # nothing was launched
    assert call(64, 64, val.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel()) == 0
    torch.cuda.synchronize()
    assert idx.tolist() == [[0, 1, 2]] * 5 and bool((val == 0).all())             # all scores tie: the lowest positions


def test_no_candidates_and_no_queries():
    y = torch.randn(5, 64, device=DEV)
    v, i = matcher_topk(torch.zeros(0, 64, device=DEV), y, 4, 0.125)
    assert bool(torch.isneginf(v).all()) and bool((i == -1).all()) and tuple(v.shape) == (5, 4)
    r = matcher_rank(torch.zeros(0, 64, device=DEV), y, torch.tensor([0, -1, 3, 0, 0], device=DEV), 0.125)
    assert r.tolist() == [-1] * 5
    v, i = matcher_topk(torch.randn(9, 64, device=DEV), torch.zeros(0, 64, device=DEV), 4, 0.125)
    assert tuple(v.shape) == (0, 4) and tuple(i.shape) == (0, 4)
    assert matcher_rank(torch.randn(9, 64, device=DEV), torch.zeros(0, 64, device=DEV), torch.zeros(0, dtype=torch.int64), 0.125).numel() == 0


def test_three_steps_of_the_example():
    spec = importlib.util.spec_from_file_location("recommend_ogbn_mag_device", os.path.join(ROOT, "examples", "recommend_ogbn_mag_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res = ex.run(steps=3, n_paper=2000, batch=48, k=10, n_hid=64, n_heads=2, n_layers=2, seed=1, device=DEV, verbose=False)
    torch.cuda.synchronize()
    A = res["n_authors"]
    assert res["cache_rows"] == A and res["ranks"].numel() == 3 * 48
    assert bool(((res["ranks"] >= 0) & (res["ranks"] < A)).all())
    assert tuple(res["indices"].shape) == (48, 10) and bool(((res["indices"] >= 0) & (res["indices"] < A)).all())
    ranks = res["ranks"].double()
    assert abs(res["mrr"] - (1.0 / (1.0 + ranks)).mean().item()) < 1e-12 and abs(res["hits10"] - (ranks < 10).double().mean().item()) < 1e-12
    # an answer's rank is its slot: the held-out author of a paper is in its top 10 exactly when its rank is below 10
    last = res["held_out"][-48:]
    in_top = (res["indices"] == last[:, None]).any(dim=1)
    assert torch.equal(in_top, res["ranks"][-48:] < 10)
