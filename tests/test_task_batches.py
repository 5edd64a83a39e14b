"""CPU tests of the task batches of the device sampler (pyhgt_amd/sampler.py): the mask that takes the label edges at the seeds out of
a sampled batch, against the reference's scripts on the fixture graph and against its own statement on the OAG-shaped graph; the
labels (`LabelSpace.targets`, the `np_label_*` siblings) against a brute-force restatement of the scripts' `pairs` / `ylabel` loops;
the argument rules of the three new C entry points.  No kernel runs here; test_task_batches_gpu.py runs the same calls on the device.

The rule: an edge of a masked triple between the sampled target of serial i and a sampled source of serial ser is left out iff
i < tgt_below or ser < src_below; serials are per type, the seeds come first."""
import ctypes as C

import numpy as np
import pytest

import test_sampler as TS
from oracle.reference_loader import reference_available, load_reference_data
from pyhgt_amd import _lib, LabelSpace, seed_edge_mask, np_label_distribution, np_label_index, np_label_counts
from pyhgt_amd.sampler import DeviceHeteroGraph, sample_subgraph_host, np_induce, TIME_NONE

G = TS.G
K = TS._tool("gen_golden_task")
TASK_RELATIONS = ["PV", "rev_PV", "PF", "rev_PF", "AP_write", "rev_AP_write"]


# ---------------------------------------------------------------------------------------------------------------- reference fixture
def _case_mask(dg, case):
    return seed_edge_mask(dg, K.task_relations(case), K.NODE_TYPE, K.batch_size(case))


def _rows_the_rule_names(rows, case):
    """rows (relation, target type, target id, source type, source id, edge time) of the unmasked fixture that the rule leaves out:
    a masked relation, and the end of the output type is one of the seeds"""
    rel_ids = [i for i, m in enumerate(G.META) if m[2] in K.task_relations(case)]
    seeds = [v[0] for v in G.CASES[case][0][K.NODE_TYPE]]
    t = G.TYPES.index(K.NODE_TYPE)
    at_seed = ((rows[:, 1] == t) & np.isin(rows[:, 2], seeds)) | ((rows[:, 3] == t) & np.isin(rows[:, 4], seeds))
    return np.isin(rows[:, 0], rel_ids) & at_seed


@pytest.mark.parametrize("case", list(G.CASES))
def test_masked_batches_equal_the_reference_fixture(case):
    edges = G.synthetic_edges()
    feats = {t: np.arange(G.N_NODES[t], dtype=np.float32).reshape(-1, 1) for t in G.TYPES}
    dg = DeviceHeteroGraph.from_csr(G.TYPES, G.META, G.N_NODES, G.csr_from_edges(edges), feats)
    det, task = np.load(G.GOLDEN), np.load(K.GOLDEN)
    inp, max_time, depth = G.CASES[case]
    res = sample_subgraph_host(dg, max_time, depth, G.SAMPLED_NUMBER, inp, seed=3, mask=_case_mask(dg, case))
    nodes, rows = TS._canonical(res)
    for t in G.TYPES:
        assert np.array_equal(nodes[t], det["%s/nodes/%s" % (case, t)]), t
    assert np.array_equal(rows, task["%s/edges" % case])
    full = det["%s/edges" % case]
    gone = _rows_the_rule_names(full, case)
    assert np.array_equal(rows, full[~gone])
    assert gone.any() == (depth > 0)                          # depth 0 samples no venue and no author: nothing to take out
    assert res.n_seed == {t: len(inp.get(t, [])) for t in G.TYPES}
    assert res.seed_rows("paper").tolist() == list(range(res[5]["paper"][0], res[5]["paper"][0] + len(inp["paper"])))
    if reference_available():
        data = load_reference_data()
        nodes_ref, rows_ref = K.run_reference_task(data, G.reference_graph(data, edges), case)
        assert np.array_equal(rows, rows_ref) and all(np.array_equal(nodes[t], nodes_ref[t]) for t in G.TYPES)


# ---------------------------------------------------------------------------------------------------------------- the OAG-shaped graph
@pytest.fixture(scope="module")
def oag():
    return TS.oag_graph()


@pytest.fixture(scope="module")
def unmasked(oag):
    """today's result of every OAG call, computed once"""
    out = []
    for call in TS.OAG_CALLS:
        res, gap, _ = TS.host_certified(oag, call)
        assert gap > TS.CERTIFIED_GAP
        out.append(res)
    return out


def _host(dg, call, mask):
    inp, max_time, depth, sn, seed = call
    return sample_subgraph_host(dg, max_time, depth, sn, inp, seed, mask=mask)


def _same_host(a, b):
    return (all(np.array_equal(u, v) for u, v in zip(a.sorted, b.sorted)) and all(np.array_equal(a.indxs[t], b.indxs[t]) for t in a.indxs)
            and all(np.array_equal(a.times[t], b.times[t]) for t in a.times) and all(np.array_equal(a[i].numpy(), b[i].numpy()) for i in range(5))
            and a[5] == b[5] and a[6] == b[6])


def oag_mask(dg, call):
    """the mask of the tests: every label relation of the three OAG tasks at the paper seeds"""
    return seed_edge_mask(dg, TASK_RELATIONS, "paper", len(call[0].get("paper", [])))


def restated_rule(dg, sorted_arrays, mask):
    """the rule applied to the sorted arrays of an unmasked result: -> (src, dst, edge_time, rel_ptr, removed per relation name)"""
    src, dst, etime, rel_ptr, type_off = [np.asarray(a) for a in sorted_arrays]
    keep, removed = np.ones(src.size, bool), {}
    for (tt, st, rel), (tgt_below, src_below) in mask.items():
        r = dg.edge_dict[rel]
        e = np.arange(rel_ptr[r], rel_ptr[r + 1])
        out = (dst[e] - type_off[dg.types.index(tt)] < tgt_below) | (src[e] - type_off[dg.types.index(st)] < src_below)
        keep[e[out]] = False
        removed[rel] = (int(out.sum()), int(e.size))
    rel_of = np.repeat(np.arange(rel_ptr.size - 1), np.diff(rel_ptr))
    new_ptr = np.concatenate([[0], np.cumsum(np.bincount(rel_of[keep], minlength=rel_ptr.size - 1))]).astype(np.int32)
    return src[keep], dst[keep], etime[keep], new_ptr, removed


def test_no_mask_empty_mask_and_zero_thresholds_are_todays_call(oag, unmasked):
    zero = {tri: (0, 0) for tri in oag.triples}
    for call, base in zip(TS.OAG_CALLS, unmasked):
        for mask in (None, {}, zero, {("paper", "venue", "PV"): (0, 0)}):
            assert _same_host(_host(oag, call, mask), base)


def test_mask_removes_exactly_the_edges_at_the_paper_seeds(oag, unmasked):
    assert len(TS.OAG_CALLS) == 22
    some, emptied, nothing = [], [], []
    for i, (call, base) in enumerate(zip(TS.OAG_CALLS, unmasked)):
        mask = oag_mask(oag, call)
        assert set(mask) == {m for m in oag.triples if m[2] in TASK_RELATIONS} and len(mask) == 6
        res = _host(oag, call, mask)
        src, dst, etime, rel_ptr, removed = restated_rule(oag, base.sorted, mask)
        for got, exp, name in zip(res.sorted, (src, dst, etime, rel_ptr, base.sorted[4]), ("src", "dst", "edge_time", "rel_ptr", "type_off")):
            assert got.dtype == np.int32 and np.array_equal(got, exp), (i, name)
        for t in oag.types:                                   # the node lists and times are untouched
            assert np.array_equal(res.indxs[t], base.indxs[t]) and np.array_equal(res.times[t], base.times[t])
        assert np.array_equal(res[0].numpy(), base[0].numpy()) and np.array_equal(res[1].numpy(), base[1].numpy())
        assert res[3].shape[1] == src.size and np.array_equal(res[3].numpy(), np.stack([src, dst]))
        assert np.array_equal(np.bincount(res[4].numpy(), minlength=len(oag.edge_dict)), np.diff(rel_ptr))
        n_self = int(base.sorted[4][-1])                      # `self` edges are never masked
        assert rel_ptr[-1] - rel_ptr[-2] == n_self
        lost = sum(k for k, _ in removed.values())
        print("call %2d: removed / edges per relation %r" % (i, removed))
        if lost == 0:
            nothing.append(i)
        elif any(k == n and n > 0 for k, n in removed.values()):
            emptied.append(i)
        else:
            some.append(i)
        if call[0] is TS._AFFIL or (call[2] == 0 and call[0] is TS._PAPERS):     # no paper among the seeds; no venue, field or author
            assert lost == 0, i
    print("lose a part: %r, a whole relation: %r, nothing: %r" % (some, emptied, nothing))
    assert some and emptied and nothing, (some, emptied, nothing)


def test_mask_arguments(oag):
    call = TS.OAG_CALLS[0]
    with pytest.raises(KeyError):
        _host(oag, call, {("paper", "venue", "no_such"): (1, 0)})
    with pytest.raises(KeyError):
        _host(oag, call, {("venue", "paper", "PV"): (1, 0)})                    # the relation exists, the triple does not
    with pytest.raises(ValueError):
        _host(oag, call, {("paper", "venue", "PV"): (-1, 0)})
    with pytest.raises(ValueError):
        _host(oag, call, {("paper", "venue", "PV"): (0, -3)})
    with pytest.raises(KeyError):
        seed_edge_mask(oag, ["PV", "nope"], "paper", 4)
    with pytest.raises(KeyError):
        seed_edge_mask(oag, ["PV"], "nope", 4)
    with pytest.raises(ValueError):
        seed_edge_mask(oag, ["PV"], "paper", -1)
    assert seed_edge_mask(oag, ["PV", "rev_PV"], "paper", 7) == {("paper", "venue", "PV"): (7, 0), ("venue", "paper", "rev_PV"): (0, 7)}
    assert seed_edge_mask(oag, ["PP_cite"], "paper", 7) == {("paper", "paper", "PP_cite"): (7, 7)}
    assert seed_edge_mask(oag, [], "paper", 7) == {}
    # np_induce is the definition and takes the same dict
    res = _host(oag, TS.OAG_CALLS[7], None)
    mask = oag_mask(oag, TS.OAG_CALLS[7])
    serial = [np.full(n, -1, np.int64) for n in oag.n_nodes]
    for t, name in enumerate(oag.types):
        serial[t][res.indxs[name]] = np.arange(len(res.indxs[name]))
    got = np_induce(oag, [res.indxs[t] for t in oag.types], [res.times[t] for t in oag.types], serial, mask)
    for a, b in zip(got, _host(oag, TS.OAG_CALLS[7], mask).sorted):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- labels
WINDOWS = {"none": (None, None), "everything": (-100, 100), "nothing": (50, 60), "part": (0, 3)}


def brute_labels(csr, cand_list, ids, t_min, t_max):
    """the scripts' loops, restated: walk the row, keep the sources that are classes and whose time is in the range, `ylabel[x][
    cand_list.index(source)] = 1`, normalise; the first kept source is the paper-venue label.  -> (dist float32 [n, C], index, count,
    time of the first kept edge or None)"""
    indptr, src, time = csr
    cand_list = list(cand_list)
    pos = {s: c for c, s in enumerate(cand_list)}
    dist, index, count, first_time = np.zeros((len(ids), len(cand_list)), np.float32), [], [], []
    for r, v in enumerate(ids):
        cols, times = [], []
        if 0 <= v < len(indptr) - 1:
            for p in range(indptr[v], indptr[v + 1]):
                s, t = int(src[p]), int(time[p])
                if s not in pos:
                    continue
                if t_min is not None and (t == TIME_NONE or not t_min <= t <= t_max):
                    continue
                cols.append(pos[s])
                times.append(t)
        for c in cols:
            dist[r, c] = 1
        if cols:
            dist[r] /= np.float32(len(set(cols)))
        index.append(cols[0] if cols else -1)
        count.append(len(set(cols)))
        first_time.append(times[0] if cols else None)
    return dist, np.array(index, np.int64), np.array(count, np.int64), first_time


def label_cases(dg):
    """name -> (triple, candidates, ids): short rows, rows on both sides of 512 with classes that cover a part of the sources, rows
    without a time, an id outside the type"""
    rng = np.random.default_rng(17)
    fields, papers = np.arange(TS.OAG_N["field"]), np.sort(rng.choice(TS.OAG_N["paper"], 1000, replace=False))
    some_papers = np.concatenate([rng.choice(TS.OAG_N["paper"], 255, replace=False), [TS.OAG_N["paper"], -1]])
    return {"PF": (("paper", "field", "PF"), rng.permutation(fields), some_papers),
            "rev_PF": (("field", "paper", "rev_PF"), rng.permutation(papers), fields),
            "PV": (("paper", "venue", "PV"), np.arange(TS.OAG_N["venue"])[::-1], some_papers[:64]),
            "rev_PV": (("venue", "paper", "rev_PV"), papers[:63], np.arange(TS.OAG_N["venue"]))}


def repeated_source_graph(device=None):
    """a <- b with sources listed twice in a row: once outside and once inside the window [6, 10], once with and once without a
    time, once with two times in the window; a row without a neighbour"""
    rows = [[(3, 5), (1, 7), (3, 9), (2, TIME_NONE), (1, 2)], [], [(4, 8), (4, 6), (0, 1)], [(2, TIME_NONE), (2, 7), (5, 7)]]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    src = np.array([s for r in rows for s, _ in r])
    tm = np.array([t for r in rows for _, t in r])
    feats = {"a": np.zeros((4, 1), np.float32), "b": np.zeros((6, 1), np.float32)}
    return DeviceHeteroGraph.from_csr(["a", "b"], [("a", "b", "ab")], {"a": 4, "b": 6}, [(indptr, src, tm)], feats, device=device)


@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("name", ["PF", "rev_PF", "PV", "rev_PV"])
def test_label_siblings_equal_the_scripts_loops(oag, name, window):
    triple, cand, ids = label_cases(oag)[name]
    t_min, t_max = WINDOWS[window]
    space = LabelSpace(oag, triple, cand)
    csr = oag.csr[oag.triples.index(triple)]
    dist, index, count, _ = brute_labels(csr, cand, ids, t_min, t_max)
    got = np_label_distribution(oag, triple, space.col_of, space.n_cols, ids, t_min, t_max)
    assert got.dtype == np.float32 and got.shape == (len(ids), len(cand)) and np.array_equal(got, dist)
    assert np.array_equal(np_label_index(oag, triple, space.col_of, ids, t_min, t_max), index)
    assert np.array_equal(np_label_counts(oag, triple, space.col_of, ids, t_min, t_max), count)
    # the host graph's LabelSpace answers with the siblings
    assert np.array_equal(space.distribution(ids, t_min, t_max).numpy(), dist) and np.array_equal(space.index(ids, t_min, t_max).numpy(), index)
    assert np.array_equal(space.counts(ids, t_min, t_max).numpy(), count)
    sums = dist.astype(np.float64).sum(axis=1)
    assert np.all((np.abs(sums - 1) < 1e-5) | (sums == 0)) and np.array_equal(sums > 0, count > 0)
    deg = np.diff(csr[0])
    if name == "PF":
        assert space.n_cols == 45 and 3 < deg.mean() < 5 and count[-2:].tolist() == [0, 0]        # the ids outside the type
    if name == "rev_PF":
        assert deg.min() < 512 < deg.max() and (space.col_of == -1).sum() == TS.OAG_N["paper"] - 1000
    if name in ("PV", "rev_PV"):                               # edges without a time: in no window, in every unwindowed call
        assert (csr[2] == TIME_NONE).all() and (count > 0).any() == (window == "none")
    elif window == "nothing":
        assert not count.any() and (index == -1).all() and not dist.any()
    elif window == "part":
        full = brute_labels(csr, cand, ids, None, None)[2]
        assert (count <= full).all() and 0 < count.sum() < full.sum()
    else:
        assert np.array_equal(count, brute_labels(csr, cand, ids, None, None)[2]) and count.sum() > 0


def test_labels_with_a_source_listed_twice_in_a_row():
    dg = repeated_source_graph()
    cand = [5, 3, 1, 4, 2]                                    # b_0 is no class
    space = LabelSpace(dg, ("a", "b", "ab"), cand)
    ids = np.arange(4)
    for t_min, t_max in [(None, None), (6, 10), (7, 7), (-5, 5)]:
        dist, index, count, _ = brute_labels(dg.csr[0], cand, ids, t_min, t_max)
        assert np.array_equal(np_label_distribution(dg, space.triple, space.col_of, 5, ids, t_min, t_max), dist)
        assert np.array_equal(np_label_index(dg, space.triple, space.col_of, ids, t_min, t_max), index)
        assert np.array_equal(np_label_counts(dg, space.triple, space.col_of, ids, t_min, t_max), count)
    assert np_label_counts(dg, space.triple, space.col_of, ids).tolist() == [3, 0, 1, 2]
    assert np_label_index(dg, space.triple, space.col_of, ids, 6, 10).tolist() == [2, -1, 3, 4]  # b_1 at 7 comes before b_3 at 9
    assert np_label_distribution(dg, space.triple, space.col_of, 5, ids, 6, 10)[0].tolist() == [0, 0.5, 0.5, 0, 0]


@pytest.mark.parametrize("name", ["PF", "rev_PF", "PV"])
def test_targets_are_the_scripts_pairs(oag, name):
    triple, cand, _ = label_cases(oag)[name]
    space = LabelSpace(oag, triple, cand)
    csr = oag.csr[oag.triples.index(triple)]
    everyone = np.arange(len(csr[0]) - 1)
    split = {}
    for window, (t_min, t_max) in {"train": (None, -1) if name != "PV" else (None, None), "valid": (0, 3), "test": (4, None)}.items():
        ids, times = space.targets(t_min, t_max)
        lo, hi = (-2 ** 31 if t_min is None else t_min), (2 ** 31 - 1 if t_max is None else t_max)
        first = brute_labels(csr, cand, everyone, None if (t_min, t_max) == (None, None) else lo, hi)[3]
        want = [(v, t) for v, t in zip(everyone, first) if t is not None]
        assert ids.dtype == np.int64 and times.dtype == np.int64
        assert list(zip(ids.tolist(), times.tolist())) == want
        split[window] = ids
    if name == "PV":
        assert len(split["train"]) == (np.diff(csr[0]) > 0).sum() > 5000 and len(split["valid"]) == 0   # no time: in no window
    else:
        assert all(len(v) for v in split.values())


def test_label_space_validates_its_candidates(oag):
    with pytest.raises(KeyError):
        LabelSpace(oag, ("paper", "venue", "rev_PV"), [0])
    with pytest.raises(IndexError):
        LabelSpace(oag, ("paper", "venue", "PV"), [0, TS.OAG_N["venue"]])
    with pytest.raises(ValueError):
        LabelSpace(oag, ("paper", "venue", "PV"), [3, 1, 3])
    with pytest.raises(ValueError):
        LabelSpace(oag, ("paper", "venue", "PV"), [3, 1]).index([0], 5, 4)
    space = LabelSpace(oag, ("paper", "venue", "PV"), [3, 1])
    assert space.n_cols == 2 and space.col_of[3] == 0 and space.col_of[1] == 1 and (space.col_of >= 0).sum() == 2


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_task_abi_argument_rules():
    """every call below returns before it launches anything (the tables point at host memory)"""
    lib = _lib.load()
    buf, p, types, triples = TS._tables()
    INV, WS = -1, -3
    masks = (_lib.HgtSamplerMask * 2)()
    masks[0], masks[1] = _lib.HgtSamplerMask(3, 0), _lib.HgtSamplerMask(0, 2 ** 31 - 1)
    count, fill = lib.hgt_sampler_induce_count_masked, lib.hgt_sampler_induce_fill_masked
    assert count(types, 2, triples, 2, 3, p, p, 8, p, p, p, masks, None) == WS                  # good masks: on to the next check
    assert count(types, 2, triples, 2, 3, p, p, 9, p, p, p, None, None) == INV
    assert count(types, 2, triples, 2, 3, None, p, 9, p, p, p, masks, None) == INV
    assert count(types, 2, triples, 2, 2, p, p, 9, p, p, p, masks, None) == INV                 # the rules of the unmasked call hold
    assert fill(types, 2, triples, 2, 3, p, p, 8, p, 4, 6, p, p, p, p, p, masks, None) == WS
    assert fill(types, 2, triples, 2, 3, p, p, 9, p, 4, 6, p, p, p, p, p, None, None) == INV
    assert fill(types, 2, triples, 2, 3, p, p, 9, p, 4, 3, p, p, p, p, p, masks, None) == INV
    for bad in (_lib.HgtSamplerMask(-1, 0), _lib.HgtSamplerMask(0, -1), _lib.HgtSamplerMask(-2 ** 31, 5)):
        for m in range(2):
            neg = (_lib.HgtSamplerMask * 2)()
            neg[m] = bad
            assert count(types, 2, triples, 2, 3, p, p, 9, p, p, p, neg, None) == INV
            assert fill(types, 2, triples, 2, 3, p, p, 9, p, 4, 6, p, p, p, p, p, neg, None) == INV
    labels = lib.hgt_sampler_labels
    tri = C.byref(triples[0])
    assert labels(tri, 8, 8, p, 0, p, 4, 0, 0, 0, p, 4, p, p, None) == 0                        # no row: nothing to do
    assert labels(None, 8, 8, p, 2, p, 4, 0, 0, 0, p, 4, p, p, None) == INV
    assert labels(tri, 8, 8, None, 2, p, 4, 0, 0, 0, p, 4, p, p, None) == INV
    assert labels(tri, 8, 8, p, 2, None, 4, 0, 0, 0, p, 4, p, p, None) == INV
    assert labels(tri, 8, 8, p, -1, p, 4, 0, 0, 0, p, 4, p, p, None) == INV
    assert labels(tri, -1, 8, p, 2, p, 4, 0, 0, 0, p, 4, p, p, None) == INV
    assert labels(tri, 8, -8, p, 2, p, 4, 0, 0, 0, p, 4, p, p, None) == INV
    assert labels(tri, 8, 8, p, 2, p, -4, 0, 0, 0, p, 4, p, p, None) == INV
    assert labels(tri, 8, 8, p, 2, p, 4, 0, 0, 0, p, 3, p, p, None) == INV                      # ld < n_cols
    assert labels(tri, 8, 8, p, 0, p, 4, 0, 0, 0, p, 3, p, p, None) == INV                      # ... also without a row
    assert labels(tri, 8, 8, p, 2, p, 4, 1, 5, 4, p, 4, p, p, None) == INV                      # t_min > t_max with a window
    assert labels(tri, 8, 8, p, 0, p, 4, 0, 5, 4, p, 4, p, p, None) == 0                        # ... which no window reads
    no_src = _lib.HgtSamplerTriple(p, None, p, 0, 1, 0, 0)
    assert labels(C.byref(no_src), 8, 8, p, 2, p, 4, 0, 0, 0, p, 4, p, p, None) == INV
    no_time = _lib.HgtSamplerTriple(p, p, None, 0, 1, 0, 0)
    assert labels(C.byref(no_time), 8, 8, p, 2, p, 4, 1, 0, 0, p, 4, p, p, None) == INV
    no_indptr = _lib.HgtSamplerTriple(None, p, p, 0, 1, 0, 0)
    assert labels(C.byref(no_indptr), 8, 8, p, 2, p, 4, 0, 0, 0, p, 4, p, p, None) == INV
    del buf
