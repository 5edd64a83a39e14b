"""The classification losses on the host: np_class_loss (pyhgt_amd/metrics.py) against the float64 torch chain of oracle/task_steps.py,
np_label_columns against np_label_distribution, what the wrappers refuse before any library call, and the declarations of the three
new entry points.  No GPU.

Gate, float64 against float64: 4 x (number of summands) x 2^-52 x sum |summand|.  A term has C summands in its logsumexp and P
label-weighted ones; a summand of the term is l_j (log l_j - (x_j - m - ls)), so sum |summand| is taken as
sum_j l_j (|log l_j| + |x_j| + |m| + |ls|).  A gradient element W p_j - l_j is bounded by max(W, 1) and carries the C summands of p."""
import os
import re

import numpy as np
import pytest
import torch

import pyhgt_amd
from oracle import task_steps as TS
from pyhgt_amd import _lib, metrics as M
from pyhgt_amd import DeviceHeteroGraph, LabelSpace, np_class_loss, np_label_columns, np_label_distribution

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = 2.0 ** -52


def make_logits(rng, n, c):
    """logits in +-30 with one entry of 80 in row 0, a row of equal logits last (n >= 3)"""
    x = rng.uniform(-30, 30, size=(n, c))
    x[0, rng.integers(c)] = 80.0
    if n >= 3:
        x[-1] = 1.5
    return x


def make_dense(rng, n, c):
    """rows with 1, 3 and C non-zeros and an all-zero row, in turn; every non-empty row sums to 1"""
    l = np.zeros((n, c))
    for r in range(n):
        k = (1, min(3, c), c, 0)[r % 4]
        if k:
            l[r, rng.choice(c, k, replace=False)] = rng.uniform(0.2, 1.0, size=k)
            l[r] /= l[r].sum()
    return l


def make_columns(rng, n, c, width):
    """lists of 0 .. min(width, C) distinct columns, ascending, -1 behind"""
    cols = np.full((n, width), -1, np.int64)
    for r in range(n):
        k = (min(width, c), 1, 0, min(width, c) // 2 + 1)[r % 4]
        cols[r, :k] = np.sort(rng.choice(c, k, replace=False))
    return cols


def term_gate(x, l):
    """float64 [n]: the float64-against-float64 gate of the terms of dense labels l (an index or a list: its dense form)"""
    x, l = np.asarray(x, np.float64), np.asarray(l, np.float64)
    m = x.max(1)
    ls = np.log(np.exp(x - m[:, None]).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.where(l > 0, l * (np.abs(np.log(l)) + np.abs(x) + np.abs(m)[:, None] + np.abs(ls)[:, None]), 0.0).sum(1)
    return 4 * (x.shape[1] + (l > 0).sum(1)) * EPS64 * mag


def dense_of(c, index=None, columns=None):
    if index is not None:
        l = np.zeros((len(index), c))
        ok = (np.asarray(index) >= 0) & (np.asarray(index) < c)
        l[np.nonzero(ok)[0], np.asarray(index)[ok]] = 1.0
        return l
    l = np.zeros((columns.shape[0], c))
    for r, row in enumerate(columns):
        ent = row[(row >= 0) & (row < c)]
        if ent.size:
            l[r, ent] = 1.0 / ent.size
    return l


def torch_chain(x, labels=None, index=None, dtype=torch.float64):
    """(terms, d sum(terms) / d x) of log_softmax + kl_div / nll_loss in `dtype` on the CPU"""
    t = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    logp = torch.log_softmax(t, dim=-1)
    terms = TS.kl_terms(logp, torch.tensor(np.asarray(labels), dtype=dtype)) if labels is not None else TS.nll_terms(logp, torch.as_tensor(index))
    terms.sum().backward()
    return terms.detach().numpy().astype(np.float64), t.grad.numpy().astype(np.float64)


@pytest.mark.parametrize("c", [1, 2, 65, 257, 4099])
def test_rule_equals_the_float64_torch_chain(c):
    rng = np.random.default_rng(c)
    n = 8
    x = make_logits(rng, n, c)
    l = make_dense(rng, n, c)
    y = rng.integers(0, c, size=n)
    for kw, dense in (({"labels": l}, l), ({"index": y}, dense_of(c, index=y))):
        terms, grad = np_class_loss(x, return_grad=True, **kw)
        want, want_grad = torch_chain(x, **kw)
        assert terms.dtype == np.float64 and terms.shape == (n,) and grad.shape == (n, c)
        err, gate = np.abs(terms - want), term_gate(x, dense)
        print("C=%d %s: worst term error %.3e (gate there %.3e)" % (c, list(kw)[0], err.max(), gate[err.argmax()]))
        assert (err <= gate).all()
        W = dense.sum(1, keepdims=True)
        assert (np.abs(grad - want_grad) <= 4 * c * EPS64 * np.maximum(W, 1.0)).all()
    assert np.array_equal(np_class_loss(x, labels=l), np_class_loss(x, labels=l, return_grad=True)[0])


@pytest.mark.parametrize("c, width", [(1, 1), (65, 8), (4099, 300)])
def test_columns_equal_the_dense_form_with_one_over_c(c, width):
    rng = np.random.default_rng(7 * c)
    n = 8
    x, cols = make_logits(rng, n, c), make_columns(rng, n, c, width)
    dense = dense_of(c, columns=cols)
    terms, grad = np_class_loss(x, columns=cols, return_grad=True)
    want, want_grad = np_class_loss(x, labels=dense, return_grad=True)
    assert (np.abs(terms - want) <= term_gate(x, dense)).all()
    assert (np.abs(grad - want_grad) <= 4 * c * EPS64).all()
    count = (cols >= 0).sum(1)
    assert np.array_equal(np_class_loss(x, columns=cols, count=count), terms) and (terms[count == 0] == 0).all()
    shuffled = cols[:, ::-1].copy()                                               # the order and the place of the padding do not matter
    assert (np.abs(np_class_loss(x, columns=shuffled) - terms) <= term_gate(x, dense)).all()


def test_special_rows_of_the_rule():
    rng = np.random.default_rng(3)
    c = 9
    x = rng.uniform(-3, 3, size=(4, c))
    # index: -1 is ignored, C is out of range
    terms, grad = np_class_loss(x, index=[-1, c, 2, c - 1], return_grad=True)
    assert terms[0] == 0 and not grad[0].any() and np.isnan(terms[1]) and np.isnan(grad[1]).all()
    assert np.isfinite(terms[2:]).all() and np.isfinite(grad[2:]).all() and np.allclose(grad[2:].sum(1), 0, atol=1e-15)
    # columns: an empty list, a column = C, a count above the width
    cols = np.array([[-1, -1, -1], [0, c, -1], [1, 2, 3], [4, -1, 5]])
    terms, grad = np_class_loss(x, columns=cols, count=[0, 2, 4, 2], return_grad=True)
    assert terms[0] == 0 and not grad[0].any()
    assert np.isnan(terms[1]) and np.isnan(terms[2]) and np.isnan(grad[1:3]).all() and np.isfinite(terms[3]) and np.isfinite(grad[3]).all()
    assert np.isfinite(np_class_loss(x, columns=cols, count=[0, 2, 3, 2])[2])
    # dense: a negative or NaN entry; an all-zero row has term 0 and gradient 0; -inf on an unlabelled column
    l = np.zeros((4, c))
    l[0, 1], l[1, 2], l[2, 3] = -0.5, np.nan, 1.0
    x[2, 5] = -np.inf
    terms, grad = np_class_loss(x, labels=l, return_grad=True)
    assert np.isnan(terms[:2]).all() and np.isnan(grad[:2]).all()
    assert np.isfinite(terms[2]) and grad[2, 5] == 0 and np.isfinite(grad[2]).all()
    assert terms[3] == 0 and not grad[3].any()
    # forms
    for kw in ({}, {"labels": l, "index": [0] * 4}, {"index": [0] * 4, "columns": cols}, {"labels": l, "count": [1] * 4}):
        with pytest.raises(ValueError):
            np_class_loss(x, **kw)
    assert np_class_loss(np.zeros((0, 5)), index=[]).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- label lists
def label_graph(device=None, n_b=140000, seed=31):
    """rows `a` with 0, 1, 5 and 300 sources (some listed twice), and a few more on both sides of the bitmap line of the label kernel;
    the tests take the first n_cols sources as the classes, column = source id"""
    rng = np.random.default_rng(seed)
    line = 131072
    rows = [[], [7], [9, 3, 9, 12, 1, 40000, 3], list(rng.choice(n_b - 1, 300, replace=False)), [line - 1, line, 5, line - 1],
            list(range(line - 40, line + 40)), [n_b - 1, n_b - 1], [0]]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    src = np.array([s for r in rows for s in r])
    tm = rng.integers(0, 10, size=src.size)
    feats = {"a": np.zeros((len(rows), 1), np.float32), "b": np.zeros((n_b, 1), np.float32)}
    return DeviceHeteroGraph.from_csr(["a", "b"], [("a", "b", "ab")], {"a": len(rows), "b": n_b}, [(indptr, src, tm)], feats, device=device)


LABEL_IDS = np.array([3, 0, 1, 2, 8, -1, 4, 5, 6, 7, 3])                          # every row, one twice, two ids outside the type


@pytest.mark.parametrize("window", [(None, None), (3, 6)])
@pytest.mark.parametrize("n_cols", [131072, 131073, 140000 - 1])
def test_label_columns_are_the_non_zero_columns_of_the_distribution(window, n_cols):
    g = label_graph()
    space = LabelSpace(g, ("a", "b", "ab"), np.arange(n_cols))
    dist = np_label_distribution(g, space.triple, space.col_of, n_cols, LABEL_IDS, *window)
    cols, count = np_label_columns(g, space.triple, space.col_of, LABEL_IDS, *window)
    assert cols.dtype == np.int32 and count.dtype == np.int32 and cols.shape == (LABEL_IDS.size, max(count.max(), 1))
    for r in range(LABEL_IDS.size):
        want = np.flatnonzero(dist[r])
        assert count[r] == want.size and np.array_equal(cols[r, :want.size], want) and (cols[r, want.size:] == -1).all()
    if window == (None, None):
        tail = {131072: [2, 40, 0, 1], 131073: [3, 41, 0, 1], 139999: [3, 80, 0, 1]}[n_cols]      # (source 139999 is no class)
        assert count[[1, 2, 3]].tolist() == [0, 1, 5] and count[4:10].tolist() == [0, 0] + tail and count[0] == count[10]
        assert count[0] == 300 if n_cols == 139999 else 250 < count[0] < 300
    # a width below the longest list keeps the first columns and the true count; a wider one pads
    for width in (1, 4, 5, 400):
        short, count_w = np_label_columns(g, space.triple, space.col_of, LABEL_IDS, *window, width=width)
        assert np.array_equal(count_w, count) and short.shape == (LABEL_IDS.size, width)
        k = min(width, cols.shape[1])
        assert np.array_equal(short[:, :k], cols[:, :k]) and (short[:, k:] == -1).all()
    got = space.columns(LABEL_IDS, *window, width=4)                              # a host graph: the numpy sibling as CPU tensors
    assert got[0].dtype == torch.int32 and np.array_equal(got[0].numpy(), np_label_columns(g, space.triple, space.col_of, LABEL_IDS, *window,
                                                                                            width=4)[0])
    with pytest.raises(ValueError):
        space.columns(LABEL_IDS, width=0)


# ---------------------------------------------------------------------------------------------------------------- wrappers
def test_wrappers_refuse_before_any_library_call(monkeypatch):
    def no_call():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", no_call)
    x = torch.zeros(3, 5)
    y = torch.zeros(3, dtype=torch.int64)
    l = torch.zeros(3, 5)
    cols = torch.zeros(3, 2, dtype=torch.int32)
    for kw in ({}, {"labels": l, "index": y}, {"index": y, "columns": cols}, {"labels": l, "index": y, "columns": cols}, {"index": y, "count": y}):
        with pytest.raises(ValueError):
            M.class_loss(x, **kw)
    with pytest.raises(ValueError):
        M.class_loss(x, index=y, reduce="batchmean")
    with pytest.raises(ValueError):
        M.class_loss(x[0], index=y)
    for bad in (x.double(), x.half(), x.numpy()):
        with pytest.raises(TypeError):
            M.class_loss(bad, index=y)
    with pytest.raises(TypeError):
        M.class_loss(x, labels=l.double())
    with pytest.raises(RuntimeError, match="np_class_loss"):
        M.class_loss(x, index=y)
    with pytest.raises(RuntimeError, match="np_class_loss"):
        M.class_loss(x, columns=cols, count=y, reduce=None)
    head = pyhgt_amd.Classifier(4, 5)
    with pytest.raises(ValueError):
        head.loss(torch.zeros(3, 4), labels=l, index=y)


# ---------------------------------------------------------------------------------------------------------------- declarations
NEW_SYMBOLS = ("hgt_class_loss", "hgt_class_loss_bwd", "hgt_sampler_label_columns")


def test_header_bindings_and_makefile_list_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    assert re.search(r"#define HGT_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    assert int(re.search(r"#define HGT_CLASS_LOSS_WAVE_COLS (\d+)", header).group(1)) == _lib.CLASS_LOSS_WAVE_COLS
    for name in NEW_SYMBOLS:
        decl = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    makefile = open(os.path.join(ROOT, "pyhgt_amd", "csrc", "Makefile")).read()
    assert "hgt_task_loss.hip" in makefile and os.path.isfile(os.path.join(ROOT, "pyhgt_amd", "csrc", "hgt_task_loss.hip"))
    lib = _lib.load()
    assert lib.hgt_abi_version() == 8 and all(hasattr(lib, name) for name in NEW_SYMBOLS)
    for name in ("class_loss", "np_class_loss", "np_label_columns"):
        assert name in pyhgt_amd.__dict__, name
    assert callable(LabelSpace.columns) and callable(pyhgt_amd.Classifier.loss)
