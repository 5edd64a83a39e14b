"""Voted evaluation on the host: np_vote_add + np_class_predict (pyhgt_amd/metrics.py) against a dict-of-vectors loop written out here
the way ogbn-mag/eval_ogbn_mag.py:148-150, 182-186 does it, the edge cases of the prediction and scoring rule, what the wrappers refuse
before any library call, and the declarations of the two new entry points.  No GPU.

tools/vote_abi_check.cpp (the argument checks of both entry points under the host sanitizers) is a stand-alone program: it is built
and run by hand with the line quoted at its top, not from here."""
import os
import re

import numpy as np
import pytest
import torch

import pyhgt_amd
from pyhgt_amd import _lib, metrics as M
from pyhgt_amd import VoteTable, np_class_predict, np_vote_add

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def test_votes_and_predictions_equal_the_dict_loop_of_the_script():
    rng = np.random.default_rng(11)
    n_nodes, n_slots, C = 40, 25, 7
    nodes = rng.permutation(n_nodes)[:n_slots]                                     # test_paper: slot i belongs to nodes[i]
    slot_of = np.full(n_nodes, -1, np.int64)
    slot_of[nodes] = np.arange(n_slots)
    silent = nodes[:3]                                                             # slots that never get a vote
    everywhere = nodes[3:8]                                                        # nodes of every piece
    others = np.setdiff1d(np.arange(n_nodes), np.concatenate([silent, everywhere]))
    pieces = [np.concatenate([everywhere, rng.choice(others, k, replace=False)]) for k in (9, 14, 6)]
    for p in pieces:
        rng.shuffle(p)
    ids = np.concatenate(pieces)
    sizes = [p.size for p in pieces]
    logits = rng.standard_normal((ids.size, C)) * 3
    assert (slot_of[ids] < 0).any() and all(np.isin(everywhere, p).all() for p in pieces)

    # the script: y_preds = {pi: zeros(C)}; per sub-graph, for pi, r in zip(yindxs, res.tolist()): y_preds[pi] += r; argmax at the end
    y_preds = {int(pi): np.zeros(C) for pi in nodes}
    seen = {int(pi): 0 for pi in nodes}
    beg = 0
    for size in sizes:
        res = log_softmax64(logits[beg:beg + size])
        for pi, r in zip(ids[beg:beg + size].tolist(), res.tolist()):
            if pi in y_preds:
                y_preds[pi] += r
                seen[pi] += 1
        beg += size

    votes, count = np.zeros((n_slots, C)), np.zeros(n_slots, np.int32)
    np_vote_add(votes, count, slot_of, logits, ids, piece_sizes=sizes)
    for i, pi in enumerate(nodes.tolist()):
        assert np.abs(votes[i] - y_preds[pi]).max() <= 1e-12 and count[i] == seen[pi]
    assert not votes[:3].any() and (count[:3] == 0).all() and (count[3:8] == 3).all()
    pred = np_class_predict(votes)
    assert pred.dtype == np.int64 and pred.tolist() == [int(y_preds[pi].argmax()) for pi in nodes.tolist()]
    # piece after piece gives the same table as one call; one piece is refused when a slotted node repeats
    again, count2, beg = np.zeros((n_slots, C)), np.zeros(n_slots, np.int32), 0
    for size in sizes:
        np_vote_add(again, count2, slot_of, logits[beg:beg + size], ids[beg:beg + size])
        beg += size
    assert np.array_equal(again, votes) and np.array_equal(count2, count)
    with pytest.raises(ValueError):
        np_vote_add(again, count2, slot_of, logits, ids)
    # labels per slot: accuracy over the voted slots
    labels = np.where(rng.random(n_slots) < 0.5, pred, (pred + 1) % C)
    _, counts = np_class_predict(votes, labels=labels, split=(count > 0).astype(np.int32) - 1)
    assert counts.tolist() == [[int((count > 0).sum()), int(((pred == labels) & (count > 0)).sum())]]


def test_float64_rule_alone_sets_almost_no_slot_aside_for_a_small_margin():
    """the condition of the end-to-end GPU test (at most 2 % of the voted slots may have a top-2 margin below twice their gate):
    N(0, 1) logits, 3 votes, C = 7; the gate of a slot is about 4 x 2^-23 x sum |logp|, a few 1e-6, against margins of order 1"""
    rng = np.random.default_rng(5)
    n, C = 4000, 7
    votes, count = np.zeros((n, C)), np.zeros(n, np.int64)
    mag = np.zeros((n, C))
    for _ in range(3):
        x = rng.standard_normal((n, C))
        np_vote_add(votes, count, np.arange(n), x, np.arange(n))
        mag += np.abs(log_softmax64(x))
    top = np.sort(votes, axis=1)
    small = (top[:, -1] - top[:, -2]) <= 2 * 4 * 2.0 ** -23 * mag.max(axis=1)
    print("slots with a margin below twice the gate: %d of %d" % (small.sum(), n))
    assert small.mean() <= 0.02 and small.sum() <= 2


def test_prediction_and_scoring_edge_cases():
    nan, inf = float("nan"), float("inf")
    x = np.array([[1, 3, 3, 2], [nan, 5, nan, 9], [-inf] * 4, [0, 1, 2, 3], [4, 4, 4, 4], [2, inf, 1, inf], [1, 2, nan, 0], [0.0, -0.0, 0, 0]],
                 np.float32)
    pred = np_class_predict(x)
    assert pred.dtype == np.int64 and pred.tolist() == [1, 0, 0, 3, 0, 1, 2, 0]
    assert np.array_equal(pred, np.argmax(x, axis=1))
    #         tie  NaN  -inf  plain  equal  inf  NaN  zeros
    labels = [1, 0, -1, 3, 0, 3, 4, 0]                                              # row 2 ignored; row 6: label >= C, scored, never correct
    p, counts = np_class_predict(x, labels=labels)
    assert np.array_equal(p, pred) and counts.dtype == np.int32 and counts.tolist() == [[7, 5]]
    split = [0, 1, 0, -1, 3, 2, 2, 1]                                               # row 3: split < 0, row 4: split >= n_splits
    _, counts = np_class_predict(x, labels=labels, split=split, n_splits=3)
    assert counts.tolist() == [[1, 1], [2, 2], [2, 0]]
    _, counts = np_class_predict(x, labels=labels, split=split, n_splits=4)
    assert counts.tolist() == [[1, 1], [2, 2], [2, 0], [1, 1]]
    # the table form equals the per-row form on the gathered arrays; ids outside the table are not scored
    rng = np.random.default_rng(2)
    table_y, table_s = rng.integers(-1, 5, size=30), rng.integers(-1, 4, size=30).astype(np.int32)
    ids = rng.integers(0, 30, size=8)
    a = np_class_predict(x, labels=table_y, split=table_s, n_splits=3, ids=ids)
    b = np_class_predict(x, labels=table_y[ids], split=table_s[ids], n_splits=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1][:, 0].sum() > 0
    out = ids.copy()
    out[[0, 5]] = [-1, 30]
    keep = np.ones(8, bool)
    keep[[0, 5]] = False
    c = np_class_predict(x, labels=table_y, split=table_s, n_splits=3, ids=out)
    d = np_class_predict(x[keep], labels=table_y[ids[keep]], split=table_s[ids[keep]], n_splits=3)
    assert np.array_equal(c[0], pred) and np.array_equal(c[1], d[1])
    # shapes and forms
    assert np_class_predict(np.zeros((0, 5), np.float32)).shape == (0,)
    assert np_class_predict(np.zeros((0, 5), np.float32), labels=[])[1].tolist() == [[0, 0]]
    for kw in ({"split": split}, {"labels": labels, "n_splits": 2}, {"labels": labels, "split": split, "n_splits": 9},
               {"labels": labels, "split": split, "n_splits": 0}, {"labels": labels[:-1]}, {"labels": labels, "ids": ids[:-1]}):
        with pytest.raises(ValueError):
            np_class_predict(x, **kw)
    with pytest.raises(ValueError):
        np_class_predict(np.zeros((3, 0), np.float32))


def test_vote_rule_skips_rows_without_a_slot_and_propagates_nan():
    C = 3
    slot_of = np.array([1, -1, 0, 5, -7])                                           # slot 5 is outside a table of two slots
    x = np.array([[0, 1, 2], [9, 9, 9], [1, 1, np.nan], [3, 3, 3], [4, 4, 4], [5, 5, 5], [6, 6, 6]], np.float64)
    ids = np.array([0, 1, 2, 3, 4, -1, 5])
    votes, count = np.ones((2, C)), np.zeros(2, np.int32)
    np_vote_add(votes, count, slot_of, x, ids)
    assert count.tolist() == [1, 1] and np.isnan(votes[0]).all() and np.allclose(votes[1], 1 + log_softmax64(x[:1])[0])
    with pytest.raises(TypeError):
        np_vote_add(np.ones((2, C), np.float32), count, slot_of, x, ids)
    with pytest.raises(ValueError):
        np_vote_add(votes, count, slot_of, x, ids, piece_sizes=[3, 3])
    with pytest.raises(ValueError):
        np_vote_add(votes, count, slot_of, x[:, :2], ids)


def test_wrappers_refuse_before_any_library_call(monkeypatch):
    def no_call():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", no_call)
    x = torch.zeros(3, 5)
    y = torch.zeros(3, dtype=torch.int64)
    s = torch.zeros(3, dtype=torch.int32)
    for bad in (x.double(), x.half(), x.numpy(), x.long()):
        with pytest.raises(TypeError):
            M.class_predict(bad)
    with pytest.raises(TypeError):
        M.class_predict(x, labels=y.float())
    for kw in ({"split": s}, {"ids": y}, {"labels": y, "n_splits": 2}, {"labels": y, "split": s, "n_splits": 9}):
        with pytest.raises(ValueError):
            M.class_predict(x, **kw)
    with pytest.raises(ValueError):
        M.class_predict(x[0])
    with pytest.raises(RuntimeError, match="np_class_predict"):
        M.class_predict(x)
    with pytest.raises(RuntimeError, match="np_class_predict"):
        M.class_predict(x, labels=y, split=s, n_splits=3)
    # the table
    with pytest.raises(ValueError):
        VoteTable(10, 5, nodes=[1, 2, 1])
    with pytest.raises(ValueError):
        VoteTable(10, 5, nodes=[1, 10])
    with pytest.raises(TypeError):
        VoteTable(10, 5, nodes=[1.0, 2.0])
    table = VoteTable(10, 5, nodes=np.array([7, 2, 4]))
    assert table.votes.shape == (3, 5) and table.votes.dtype == torch.float32 and not table.votes.any()
    assert table.count.dtype == torch.int32 and table.count.tolist() == [0, 0, 0] and table.nodes.tolist() == [7, 2, 4]
    assert table.slot_of.dtype == torch.int32 and table.slot_of.tolist() == [-1, -1, 1, -1, 2, -1, -1, 0, -1, -1]
    assert VoteTable(4, 2).slot_of.tolist() == [0, 1, 2, 3]
    with pytest.raises(TypeError):
        table.add(x.double(), y)
    with pytest.raises(ValueError):
        table.add(torch.zeros(3, 4), y)
    with pytest.raises(RuntimeError, match="np_vote_add"):
        table.add(x, y)
    with pytest.raises(RuntimeError, match="np_class_predict"):
        table.predict()
    head = pyhgt_amd.Classifier(4, 5)
    with pytest.raises(RuntimeError, match="np_vote_add"):
        head.vote(torch.zeros(3, 4), table, y)
    with pytest.raises(RuntimeError, match="np_class_predict"):
        head.predict(torch.zeros(3, 4), labels=y)


NEW_SYMBOLS = ("hgt_class_predict", "hgt_vote_add")


def test_header_bindings_and_makefile_list_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    assert re.search(r"#define HGT_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    assert int(re.search(r"#define HGT_PREDICT_MAX_SPLITS (\d+)", header).group(1)) == _lib.PREDICT_MAX_SPLITS == 8
    for name in NEW_SYMBOLS:
        decl = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    makefile = open(os.path.join(ROOT, "pyhgt_amd", "csrc", "Makefile")).read()
    assert "hgt_task_vote.hip" in makefile and os.path.isfile(os.path.join(ROOT, "pyhgt_amd", "csrc", "hgt_task_vote.hip"))
    lib = _lib.load()
    assert lib.hgt_abi_version() == 8 and all(hasattr(lib, name) for name in NEW_SYMBOLS)
    for name in ("class_predict", "VoteTable", "np_class_predict", "np_vote_add"):
        assert name in pyhgt_amd.__dict__, name
    assert callable(pyhgt_amd.Classifier.predict) and callable(pyhgt_amd.Classifier.vote)
    check = open(os.path.join(ROOT, "tools", "vote_abi_check.cpp")).read()
    assert "-fsanitize=address,undefined" in check and "int main()" in check and all(name in check for name in NEW_SYMBOLS)
