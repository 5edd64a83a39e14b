"""The voted-evaluation kernels (csrc/hgt_task_vote.hip) on the GPU against the rules of pyhgt_amd/metrics.py on the same inputs.

Predictions and counts are integers: they equal np.argmax / np_class_predict exactly.

Gate of a vote table (derived, not chosen; float32 device sums against the float64 rule np_vote_add), per element:
  4 x max(E_torch, 2^-23 x (|V0| + sum_k |logp_k|))
E_torch is the error of torch's own float32 CPU chain, v[slots] += log_softmax(x32) piece after piece in the same order, against
float64 -- another rounding of the same sums is as legitimate as torch's -- and the floor, one float32 rounding of everything that is
added into the element, keeps elements alive on which torch happens to be exact.
Measured on an MI355X (pytest -s prints them): the worst vote error over every case of the vote test was 1.3e-06 under a gate of
3.9e-06 there (C = 349); the example's tables, 44 test papers: variance_reduce 1.0e-06 under 2.9e-06, sequential 2.9e-07 under 7.1e-07,
no slot set aside for a small margin in either mode."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_class_loss_gpu import place
from pyhgt_amd import _lib, model, Classifier, VoteTable, class_predict, np_class_predict, np_vote_add

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
W = _lib.CLASS_LOSS_WAVE_COLS
EPS32 = 2.0 ** -23
SIZES = [1, 2, 63, 64, 65, W - 1, W, W + 1, 1023, 1024, 1025, 4099, 20011]
WORST = {"vote": (0.0, 0.0)}


# ---------------------------------------------------------------------------------------------------------------- 1. argmax
def argmax_rows(c, seed):
    """37 rows of C float32: random ones, the maximum planted twice (first / last, 63 / 64, W - 1 / W, two 1024-column chunks), an
    all-equal row, one and two NaNs, a row of -inf, a row with +inf"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((37, c)).astype(np.float32)
    below = np.nextafter(np.float32(50.0), np.float32(0))
    pairs = ((0, c - 1), (63, 64), (W - 1, W), (5, 1024 + 5), (1023, 2048), (1024 + 700, 3 * 1024 + 1), (c // 2, c // 2 + 1), (c // 3, c - 2))
    for r, (lo, hi) in zip(range(8, 24, 2), pairs):
        if 0 <= lo < hi < c:
            x[r, [lo, hi]] = 50.0                                                  # the lower position wins
            x[r + 1, [lo, hi]] = [below, 50.0]                                     # the nearly-equal one loses
    x[30] = -3.25
    x[31, rng.integers(c)] = np.nan
    x[32, [rng.integers(c), rng.integers(c)]] = np.nan
    x[33, [0, c - 1]] = np.nan
    x[34] = -np.inf
    x[35, rng.integers(c)] = np.inf
    x[36, [c - 1, c // 3]] = [np.inf, np.nan]
    return x


@pytest.mark.parametrize("layout", ["contiguous", "odd slice"])
@pytest.mark.parametrize("c", SIZES)
def test_class_predict_is_np_argmax(c, layout):
    x = argmax_rows(c, 17 * c)
    pred = class_predict(place(x, layout))
    assert pred.dtype == torch.int64 and pred.shape == (37,) and pred.device.type == "cuda"
    want = np.argmax(x, axis=1)
    assert np.array_equal(want, np_class_predict(x))
    assert np.array_equal(pred.cpu().numpy(), want), np.flatnonzero(pred.cpu().numpy() != want)
    one = class_predict(place(x[5:6], layout))                                     # a row alone, and the rows in another geometry
    assert one.item() == want[5]


# ---------------------------------------------------------------------------------------------------------------- 2. counts
def raw_predict(x, n_cols, ids=None, n_table=0, label=None, split=None, n_splits=1, counts=None, want_pred=True):
    lib, n = _lib.load(), x.shape[0]
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    pred = torch.full((n,), -9, dtype=torch.int64, device=DEV) if want_pred else None
    rc = lib.hgt_class_predict(ptr(x), x.stride(0) if n else n_cols, n, n_cols, ptr(ids), n_table, ptr(label), ptr(split), n_splits, ptr(pred),
                               ptr(counts), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "hgt_class_predict")
    return pred


@pytest.mark.parametrize("n_rows", [0, 1, 65, 1000])
@pytest.mark.parametrize("n_splits", [1, 3, 8])
def test_counts_are_exact_in_both_label_forms(n_splits, n_rows):
    c, n_table = 349, 500
    rng = np.random.default_rng(100 * n_splits + n_rows)
    x = rng.standard_normal((n_rows, c)).astype(np.float32)
    table_y = rng.integers(-2, c + 2, size=n_table)                                # ignored labels (< 0) and labels >= C
    hit = rng.random(n_table) < 0.5
    table_s = rng.integers(-1, n_splits + 1, size=n_table).astype(np.int32)         # splits below 0 and >= n_splits
    ids = rng.integers(-3, n_table + 3, size=n_rows)                               # ids outside the table
    inside = (ids >= 0) & (ids < n_table)
    if n_rows:                                                                     # about half of the rows carry their own prediction
        mine = np.argmax(x, axis=1)
        at = ids[inside]
        table_y[at[hit[at]]] = mine[inside][hit[at]]
    row_y = np.where(inside, table_y[np.clip(ids, 0, n_table - 1)], -1)
    row_s = np.where(inside, table_s[np.clip(ids, 0, n_table - 1)], -1).astype(np.int32)
    want_pred, want = np_class_predict(x, labels=table_y, split=table_s, n_splits=n_splits, ids=ids)
    assert np.array_equal(want, np_class_predict(x, labels=row_y, split=row_s, n_splits=n_splits)[1])
    if n_rows >= 65:
        assert (want[:, 0] > 0).all() and want[:, 1].sum() > 0 and (want[:, 1] < want[:, 0]).any()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xd, ty, ts, ry, rs, idd = dev(x), dev(table_y), dev(table_s), dev(row_y), dev(row_s), dev(ids)
    results = []
    for kw in (dict(ids=idd, n_table=n_table, label=ty, split=ts), dict(label=ry, split=rs)) * 2:
        if n_rows == 0 and "ids" not in kw:
            kw = dict(label=ty, split=ts)                                          # (a label array there must be: any device array)
        counts = torch.full((n_splits, 2), 0x5A5A5A5A, dtype=torch.int32, device=DEV)      # garbage: the call must not need zeros
        pred = raw_predict(xd, c, n_splits=n_splits, counts=counts, **kw)
        assert np.array_equal(pred.cpu().numpy(), want_pred) and np.array_equal(counts.cpu().numpy(), want), kw.keys()
        results.append((pred, counts))
    assert all(torch.equal(a, b) for a, b in zip(results[0], results[2])) and all(torch.equal(a, b) for a, b in zip(results[1], results[3]))
    # counts alone, without the predictions
    if n_rows:
        counts = torch.full((n_splits, 2), -1, dtype=torch.int32, device=DEV)
        assert raw_predict(xd, c, label=ry, split=rs, n_splits=n_splits, counts=counts, want_pred=False) is None
        assert np.array_equal(counts.cpu().numpy(), want)
    # the wrapper: both forms, and without `split` every labelled row goes to split 0
    for kw in (dict(labels=ty, split=ts, ids=idd), dict(labels=ry, split=rs)):
        pred, counts = class_predict(xd, n_splits=n_splits, **kw)
        assert counts.dtype == torch.int32 and counts.shape == (n_splits, 2) and counts.device.type == "cuda"
        assert np.array_equal(pred.cpu().numpy(), want_pred) and np.array_equal(counts.cpu().numpy(), want)
    if n_splits == 1:
        pred, counts = class_predict(xd, labels=ty, ids=idd)
        assert np.array_equal(counts.cpu().numpy(), np_class_predict(x, labels=table_y, ids=ids)[1])
        assert counts[0, 0].item() == (row_y >= 0).sum()


# ---------------------------------------------------------------------------------------------------------------- 3. votes
def slotted_rows(ids, slot_of):
    """the rows whose id lies inside the graph and has a slot"""
    inside = (ids >= 0) & (ids < slot_of.size)
    return np.flatnonzero(inside & (slot_of[np.where(inside, ids, 0)] >= 0))


def torch32_votes(v0, slot_of, calls):
    """torch's float32 CPU chain on a copy of the table v0 [n_slots, C]: per piece v[slots] += log_softmax(x32)[rows], in order"""
    v = torch.from_numpy(v0.copy())
    for x, ids, sizes in calls:
        logp = torch.log_softmax(torch.from_numpy(x), dim=-1)
        inside = (ids >= 0) & (ids < slot_of.size)
        slot = np.where(inside, slot_of[np.where(inside, ids, 0)], -1)
        has, beg = (slot >= 0) & (slot < v0.shape[0]), 0
        for size in sizes:
            rows = np.arange(beg, beg + size)[has[beg:beg + size]]
            v[torch.from_numpy(slot[rows])] += logp[torch.from_numpy(rows)]
            beg += size
    return v.numpy().astype(np.float64)


def vote_gate(v0, slot_of, calls):
    """-> (float64 table of the rule, its counts, the per-element gate of the module docstring)"""
    want, count, mag = v0.astype(np.float64), np.zeros(v0.shape[0], np.int32), np.abs(v0.astype(np.float64))
    for x, ids, sizes in calls:
        np_vote_add(want, count, slot_of, x, ids, piece_sizes=sizes)
        x64 = x.astype(np.float64)
        m = x64.max(axis=1, keepdims=True)
        logp = x64 - m - np.log(np.exp(x64 - m).sum(axis=1, keepdims=True))
        inside = (ids >= 0) & (ids < slot_of.size)
        slot = np.where(inside, slot_of[np.where(inside, ids, 0)], -1)
        has = (slot >= 0) & (slot < v0.shape[0])
        np.add.at(mag, slot[has], np.abs(logp[has]))
    e_torch = np.abs(torch32_votes(v0, slot_of, calls) - want)
    return want, count, 4 * np.maximum(e_torch, EPS32 * mag)


@functools.lru_cache(maxsize=None)
def vote_case(c, layout):
    """3 pieces of 50, 0 and 31 rows over 120 nodes and 70 slots; the table is the first C columns of a [70, C + 3] tensor of random
    float32.  -> everything the vote tests look at, computed once per (C, layout)"""
    rng = np.random.default_rng(31 * c)
    n_nodes, n_slots, sizes = 120, 70, [50, 0, 31]
    nodes = rng.permutation(n_nodes)[:n_slots]
    slot_of = np.full(n_nodes, -1, np.int64)
    slot_of[nodes] = np.arange(n_slots)
    bare = np.setdiff1d(np.arange(n_nodes), nodes)
    outside = np.array([-1, n_nodes, 2 ** 40, -5, n_nodes + 7, -2 ** 40])
    first = np.concatenate([nodes[:40], rng.choice(bare, 6), outside[:4]])          # 40 slotted, distinct
    second = np.concatenate([nodes[28:53], rng.choice(bare, 4), outside[4:]])       # 25 slotted, 12 of them in the first piece too
    rng.shuffle(first), rng.shuffle(second)
    ids = np.concatenate([first, second])
    assert ids.size == sum(sizes) and np.intersect1d(first, second).size >= 12
    x = (rng.standard_normal((ids.size, c)) * 3).astype(np.float32)
    wide0 = rng.standard_normal((n_slots, c + 3)).astype(np.float32)
    v0 = np.ascontiguousarray(wide0[:, :c])

    def fresh():
        table = VoteTable(n_nodes, c, nodes=nodes, device=DEV)
        wide = torch.from_numpy(wide0).to(DEV)
        table.votes = wide[:, :c]                                                  # ld_votes = C + 3: three padding columns a row
        return table, wide

    xd, idd = place(x, layout), torch.from_numpy(ids).to(DEV)
    table, wide = fresh()
    assert table.add(xd, idd, piece_sizes=sizes, check=True) is table
    torch.cuda.synchronize()
    return dict(c=c, nodes=nodes, slot_of=slot_of, ids=ids, sizes=sizes, x=x, xd=xd, idd=idd, v0=v0, wide0=wide0, fresh=fresh, table=table,
                wide=wide)


VOTE_SIZES = [1, 64, W, W + 1, 349, 1025, 4099]


@pytest.mark.parametrize("layout", ["contiguous", "odd slice"])
@pytest.mark.parametrize("c", VOTE_SIZES)
def test_vote_add_against_the_float64_rule(c, layout):
    K = vote_case(c, layout)
    sizes, ids, x, slot_of, v0 = K["sizes"], K["ids"], K["x"], K["slot_of"], K["v0"]
    want, want_count, gate = vote_gate(v0, slot_of, [(x, ids, sizes)])
    got = K["wide"].cpu().numpy()
    err = np.abs(got[:, :c].astype(np.float64) - want)
    at = np.unravel_index((err / gate).argmax() if c > 1 else err.argmax(), err.shape)
    print("C=%d %s: worst vote error %.3e (gate there %.3e)" % (c, layout, err[at], gate[at]))
    if err[at] > WORST["vote"][0]:
        WORST["vote"] = (err[at], gate[at])
    print("worst so far: %.3e under %.3e" % WORST["vote"])
    assert np.isfinite(got).all() and (err <= gate).all()
    count = K["table"].count.cpu().numpy()
    assert count.dtype == np.int32 and np.array_equal(count, want_count) and sorted(set(count.tolist())) == [0, 1, 2]
    # untouched slots and the three padding columns of every row: the bits they had
    assert np.array_equal(got[:, c:].view(np.uint32), K["wide0"][:, c:].view(np.uint32))
    assert np.array_equal(got[count == 0].view(np.uint32), K["wide0"][count == 0].view(np.uint32))
    # one call with piece_sizes = the single-piece calls one after another; the same sequence again = the same bits
    table, wide = K["fresh"]()
    beg = 0
    for size in sizes:
        table.add(K["xd"][beg:beg + size], K["idd"][beg:beg + size])
        beg += size
    assert torch.equal(wide, K["wide"]) and torch.equal(table.count, K["table"].count)
    table, wide = K["fresh"]()
    table.add(K["xd"], K["idd"], piece_sizes=sizes)
    assert torch.equal(wide, K["wide"]) and torch.equal(table.count, K["table"].count)
    # a NaN logit makes exactly its slot's row NaN
    row = int(slotted_rows(ids, slot_of)[3])
    bad = x.copy()
    bad[row, c // 2] = np.nan
    table, wide = K["fresh"]()
    table.add(place(bad, layout), K["idd"], piece_sizes=sizes)
    nan = torch.isnan(table.votes).cpu().numpy()
    assert nan[slot_of[ids[row]]].all() and nan.sum() == c and not torch.isnan(wide[:, c:]).any()
    # a planted duplicate inside a piece: refused by check=True (before the launch)
    twice = ids.copy()
    slotted = slotted_rows(twice[:50], slot_of)
    twice[slotted[1]] = twice[slotted[0]]
    table, wide = K["fresh"]()
    with pytest.raises(ValueError):
        table.add(K["xd"], torch.from_numpy(twice).to(DEV), piece_sizes=sizes, check=True)
    assert torch.equal(wide, torch.from_numpy(K["wide0"]).to(DEV)) and not table.count.any()
    table.add(K["xd"], torch.from_numpy(twice).to(DEV), piece_sizes=[slotted[1]] + [50 - slotted[1], 0, 31], check=True)      # apart: fine


# ---------------------------------------------------------------------------------------------------------------- 4. the table's answer
@pytest.mark.parametrize("c", VOTE_SIZES)
def test_vote_table_predict_and_accuracy(c):
    K = vote_case(c, "contiguous")
    table = K["table"]
    votes, count = table.votes.cpu().numpy(), table.count.cpu().numpy()
    want = np.where(count > 0, np.argmax(votes, axis=1), -1)
    pred = table.predict()
    assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), want) and (want == -1).sum() == (count == 0).sum() > 0
    rng = np.random.default_rng(c)
    labels = np.where(rng.random(want.size) < 0.6, np.argmax(votes, axis=1), rng.integers(0, c, size=want.size))
    labels[:4] = -1                                                                # unlabelled slots are not scored
    pred2, pair = table.predict(torch.from_numpy(labels).to(DEV))
    scored = (count > 0) & (labels >= 0)
    assert torch.equal(pred2, pred) and pair.dtype == torch.int32 and pair.device.type == "cuda"
    assert pair.tolist() == [int(scored.sum()), int((scored & (want == labels)).sum())]
    assert table.accuracy(labels) == (scored & (want == labels)).sum() / scored.sum()
    empty = VoteTable(120, c, nodes=K["nodes"], device=DEV)
    assert (empty.predict() == -1).all() and np.isnan(empty.accuracy(labels))
    table2, _ = K["fresh"]()
    table2.add(K["xd"], K["idd"], piece_sizes=K["sizes"])
    table2.reset()
    assert not table2.votes.any() and not table2.count.any()


# ---------------------------------------------------------------------------------------------------------------- 5. Classifier
def test_classifier_predict_and_vote_are_the_calls_on_its_logits():
    n, n_hid, c = 65, 64, 349
    rng = np.random.default_rng(9)
    torch.manual_seed(9)
    head = Classifier(n_hid, c).to(DEV)
    x = torch.from_numpy(rng.standard_normal((n, n_hid)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        logits = model._dense_linear(x, head.linear.weight, head.linear.bias)
        assert torch.allclose(logits, torch.nn.functional.linear(x, head.linear.weight, head.linear.bias), atol=1e-4)
    y = torch.from_numpy(rng.integers(-1, c, size=500)).to(DEV)
    split = torch.from_numpy(rng.integers(-1, 4, size=500).astype(np.int32)).to(DEV)
    ids = torch.from_numpy(rng.permutation(500)[:n]).to(DEV)
    for xx in (x, x.clone().requires_grad_()):
        pred, counts = head.predict(xx, ids=ids, labels=y, split=split, n_splits=3)
        want_pred, want_counts = class_predict(logits, ids=ids, labels=y, split=split, n_splits=3)
        assert torch.equal(pred, want_pred) and torch.equal(counts, want_counts) and not pred.requires_grad
        assert torch.equal(head.predict(xx), want_pred) and torch.equal(head.logits(xx), logits)
    nodes = rng.permutation(500)[:200]
    a, b = VoteTable(500, c, nodes=nodes, device=DEV), VoteTable(500, c, nodes=nodes, device=DEV)
    for _ in range(2):
        assert head.vote(x, a, ids, piece_sizes=[40, 25]) is a
        b.add(logits, ids, piece_sizes=[40, 25])
    assert torch.equal(a.votes, b.votes) and torch.equal(a.count, b.count) and a.count.max().item() == 2


# ---------------------------------------------------------------------------------------------------------------- 6. the example
def test_ogbn_mag_example_end_to_end_at_the_smallest_size():
    spec = importlib.util.spec_from_file_location("train_eval_ogbn_mag_device", os.path.join(ROOT, "examples", "train_eval_ogbn_mag_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    c, trace = 7, {}
    losses, accs, tables = ex.run(steps=2, n_paper=400, n_classes=c, n_hid=64, n_heads=4, n_layers=2, batch_size=16, depth=2, width=8, vr_num=3,
                                  verbose=False, device=DEV, trace=trace)
    _, n_nodes, _, y, split = ex.task_graph(400, 129, c, None)
    assert len(losses) == 2 and np.isfinite(losses).all() and len(trace["steps"]) == 2
    for acc, (logits, ids) in zip(accs, trace["steps"]):
        counts = np_class_predict(logits.numpy(), labels=y, split=split, n_splits=3, ids=ids.numpy())[1]
        assert counts[0, 0] >= 16 and ids.numel() > 16
        want = [k / n if n else float("nan") for n, k in counts.tolist()]
        assert np.array_equal(np.array(acc), np.array(want), equal_nan=True), (acc, want)
    for mode, table in tables.items():
        nodes = table.nodes.cpu().numpy()
        assert np.array_equal(np.sort(nodes), np.flatnonzero(split == 2)) and len(trace["votes"][mode]) == -(-nodes.size // 16)
        slot_of = table.slot_of.cpu().numpy().astype(np.int64)
        calls = [(x.numpy(), ids.numpy(), sizes) for x, ids, sizes in trace["votes"][mode]]
        assert all(len(sizes) == (3 if mode == "variance_reduce" else 1) for _, _, sizes in calls)
        want, want_count, gate = vote_gate(np.zeros((nodes.size, c), np.float32), slot_of, calls)
        got, count = table.votes.cpu().numpy().astype(np.float64), table.count.cpu().numpy()
        err = np.abs(got - want)
        at = np.unravel_index((err / gate).argmax(), err.shape)
        print("%s: %d test papers, %d voted, worst vote error %.3e (gate there %.3e)" % (mode, nodes.size, (count > 0).sum(), err[at], gate[at]))
        assert np.array_equal(count, want_count) and (count > 0).all() and (err <= gate).all()
        top = np.sort(want, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 2 * gate.max(axis=1)
        voted = count > 0
        print("%s: %d of %d voted slots set aside for a small margin" % (mode, (voted & ~clear).sum(), voted.sum()))
        assert (voted & ~clear).sum() <= 0.02 * voted.sum()
        pred = table.predict().cpu().numpy()
        assert np.array_equal(pred[voted & clear], np.argmax(want, axis=1)[voted & clear])
        y_test = y[nodes]
        assert table.accuracy(torch.from_numpy(y_test).to(DEV)) == (pred == y_test)[voted].mean()
