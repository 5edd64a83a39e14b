"""The whole-graph view's definition (pyhgt_amd.view.np_whole_graph) on the CPU: against the reference's own sample_subgraph +
to_torch with every node a seed (live where the reference tree is present, and against the committed output of that run everywhere),
against a brute-force loop over nested dicts on a hand-made graph, and `label_edge_flags` against `seed_edge_mask`."""
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

from oracle.reference_loader import reference_available, load_reference_data
from pyhgt_amd import np_whole_graph, label_edge_flags, seed_edge_mask, sample_subgraph_host
from pyhgt_amd.sampler import DeviceHeteroGraph

import whole_graph_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


V = _tool("gen_golden_view")
G = V.G


@pytest.fixture(scope="module")
def small():
    edges = G.synthetic_edges()
    feats = {t: np.arange(G.N_NODES[t], dtype=np.float32).reshape(-1, 1) for t in G.TYPES}
    return edges, DeviceHeteroGraph.from_csr(G.TYPES, G.META, G.N_NODES, G.csr_from_edges(edges), feats)


def _equals_reference_output(dg, nf, nt, rows, node_dict, edge_dict):
    a = np_whole_graph(dg, node_time=V.node_times())
    assert np.array_equal(a.node_feature, nf) and np.array_equal(a.node_type, nt)
    assert np.array_equal(V.edge_rows(a.edge_index, a.edge_type, a.edge_time), rows)
    assert a.node_dict == node_dict and a.edge_dict == edge_dict
    assert list(a.node_dict) == list(node_dict) and list(a.edge_dict) == list(edge_dict)


def test_definition_equals_the_committed_reference_output(small):
    """np_whole_graph against what the reference's sample_subgraph (sampled_depth = 0, every node a seed in id order with its
    node_time) + to_torch returned: the node arrays, the multiset of (source, target, edge_type, edge_time), the two dictionaries"""
    _, dg = small
    fx = np.load(V.GOLDEN)
    as_dict = lambda k: {str(n): (v.tolist() if v.ndim else int(v)) for n, v in zip(fx[k + "/names"], fx[k + "/values"])}
    _equals_reference_output(dg, fx["node_feature"], fx["node_type"], fx["edges"], as_dict("node_dict"), as_dict("edge_dict"))
    assert len(fx["edges"]) > sum(G.N_NODES.values()) and (fx["edges"][:, 3] != 120).any()      # not only self loops, real time gaps


@pytest.mark.skipif(not reference_available(), reason="the reference tree is not present")
def test_definition_equals_the_live_reference(small):
    edges, dg = small
    data = load_reference_data()
    nf, nt, rows, node_dict, edge_dict = V.run_reference(data, G.reference_graph(data, edges))
    _equals_reference_output(dg, nf, nt, rows, node_dict, edge_dict)
    assert np.array_equal(rows, np.load(V.GOLDEN)["edges"])


# ---------------------------------------------------------------------------------------------------- order and filter rules
@pytest.mark.parametrize("with_time,max_time,flags,self_loops",
                         list(itertools.product([True, False], [None, W.HAND_MAX_TIME], [None, "targets", "sources", "both"], [True, False])))
def test_order_and_filters_equal_the_brute_force_loop(with_time, max_time, flags, self_loops):
    """Hand-made graph (tests/whole_graph_cases.py: a shared relation name, a type without nodes, empty triples, empty rows at the
    start, middle and end, None times): every array in order against a loop over the nested dicts"""
    dg = W.hand_graph()
    node_time = W.HAND_TIME if with_time else None
    leave_out = None if flags is None else W.hand_flags(flags)
    a = np_whole_graph(dg, node_time, max_time, leave_out, self_loops)
    edges, rel_ptr = W.brute_force(dg, W.HAND_NESTED, node_time, max_time, leave_out, self_loops)
    W.check_against(a, edges, rel_ptr, with_time)
    assert np.array_equal(a.node_type, np.repeat([0, 1, 3], [6, 5, 3]))
    assert a.node_dict == {"a": [0, 0], "b": [6, 1], "c": [11, 2], "d": [11, 3]} and a.edge_dict == dg.edge_dict
    assert np.array_equal(a.sorted[4], [0, 6, 11, 11, 14])
    assert np.array_equal(a.node_feature[:, 0], np.concatenate([1000 * i + np.arange(n) for i, n in enumerate(dg.n_nodes)]))


def test_filters_do_what_they_say():
    """the cases are not trivial: the filters drop something, None entries go both ways, nodes are never dropped"""
    dg = W.hand_graph()
    count = lambda **kw: np_whole_graph(dg, **kw).edge_index.shape[1]
    full = count()
    assert full == 17 + 14 and count(self_loops=False) == 17
    assert count(max_time=W.HAND_MAX_TIME) == full - 6                                  # None entries kept without tables
    assert count(max_time=W.HAND_MAX_TIME, node_time=W.HAND_TIME) == full - 6 - 3      # a3 (2003), b2 (2002): newer; d2 (2000): kept
    for kind in ("targets", "sources", "both"):
        assert count(leave_out=W.hand_flags(kind)) < full
    a = np_whole_graph(dg, max_time=1900, node_time=W.HAND_TIME)
    assert a.edge_index.shape[1] == 14 and a.node_type.size == 14 and np.array_equal(a.sorted[3], [0, 0, 0, 0, 0, 0, 14])


def test_entry_rule_truth_table():
    """_np_kept / _np_time_diff, the one numpy statement of the entry rule both np_whole_graph and np_neighbourhood call, entry by
    entry against a loop written out here: stored time below / at / above max_time / TIME_NONE x target table absent / target time
    <= max_time / > max_time x target flag x source flag x max_time None / given (and each flag array absent)."""
    from pyhgt_amd.sampler import TIME_NONE
    from pyhgt_amd.view import _np_kept, _np_time_diff
    MAX = 2000
    tgt_table = np.array([MAX, MAX, MAX + 5, MAX + 5], np.int64)          # target nodes: time <= / > max_time x flag unset / set
    tf, sf = np.array([0, 1, 0, 1], bool), np.array([0, 1], np.uint8)
    stored, rows, src = (np.array(x) for x in zip(*itertools.product([MAX - 1, MAX, MAX + 1, TIME_NONE], range(4), range(2))))
    stored = stored.astype(np.int32)

    def kept(st, r, s, tgt_times, max_time, flags):
        if max_time is not None:
            if st == TIME_NONE:                                           # the entry takes the target's time, if there is one
                if tgt_times is not None and tgt_times[r] > max_time:
                    return False
            elif st > max_time:
                return False
        if flags is not None and flags[0] is not None and flags[0][r]:
            return False
        if flags is not None and flags[1] is not None and flags[1][s]:
            return False
        return True

    seen = set()
    for tgt_times, max_time, flags in itertools.product([None, tgt_table], [None, MAX], [None, (tf, sf), (tf, None), (None, sf)]):
        got = _np_kept(stored, rows, src, tgt_times, max_time, flags)
        want = [kept(st, r, s, tgt_times, max_time, flags) for st, r, s in zip(stored.tolist(), rows, src)]
        assert got.dtype == bool and got.tolist() == want, (tgt_times, max_time, flags)
        seen.update(want)
    assert seen == {True, False}
    # the time difference: 0 and 239 are the ends of the RTE table, -1 and 240 lie outside
    tt, st = np.array([2000, 2100], np.int64), np.array([2120, 1981, 2000], np.int64)
    r, s = np.array([0, 1, 0, 1]), np.array([0, 1, 2, 2])
    dt = _np_time_diff(tt, st, r, s, "whole_graph: a time difference of ('a', 'b', 'link')")
    assert dt.dtype == np.int64 and dt.tolist() == [0, 239, 120, 220]
    assert _np_time_diff(tt, st, r[:0], s[:0], "whole_graph").size == 0
    for what, src_time in (("whole_graph", 2121), ("neighbourhood", 1880)):        # 2000 - 2121 + 120 = -1; 2000 - 1880 + 120 = 240
        with pytest.raises(IndexError, match=what + r".*outside \[0, 240\)"):
            _np_time_diff(tt, np.array([src_time], np.int64), np.array([0]), np.array([0]), what + ": a time difference of x")


def test_argument_errors():
    dg = W.hand_graph()
    with pytest.raises(ValueError):
        np_whole_graph(dg, node_time={"a": W.HAND_TIME["a"], "b": W.HAND_TIME["b"]})    # partial: "d" has nodes
    with pytest.raises(ValueError):
        np_whole_graph(dg, node_time=dict(W.HAND_TIME, a=W.HAND_TIME["a"][:5]))
    late = dict(W.HAND_TIME, b=W.HAND_TIME["b"] + 121)                                  # a1 <- b0: 2001 - 2122 + 120 < 0
    with pytest.raises(IndexError):
        np_whole_graph(dg, node_time=late)
    early = dict(W.HAND_TIME, b=W.HAND_TIME["b"] - 121)                                 # a3 <- b1: 2003 - 1879 + 120 >= 240
    with pytest.raises(IndexError):
        np_whole_graph(dg, node_time=early)
    # ... but not when the filter drops the offending edges: the test is on kept edges
    flag_b = np.ones(5, bool)
    drop = {tri: ((flag_b if tri[0] == "b" else None), (flag_b if tri[1] == "b" else None)) for tri in dg.triples if "b" in tri[:2]}
    assert np_whole_graph(dg, node_time=late, leave_out=drop).edge_index.shape[1] == 4 + 3 + 14
    with pytest.raises(KeyError):
        np_whole_graph(dg, leave_out={("a", "d", "link"): (None, None)})
    with pytest.raises(ValueError):
        np_whole_graph(dg, leave_out={("a", "b", "link"): (np.zeros(5, bool), None)})   # flags over the wrong type
    assert np_whole_graph(dg, node_time={}).edge_time is None
    np_whole_graph(dg, node_time=dict(W.HAND_TIME, c=np.zeros(0, np.int64)))          # a table for the empty type is fine


def test_host_graph_returns_the_definition_as_cpu_tensors():
    dg = W.hand_graph()
    leave_out = W.hand_flags("both")
    a = np_whole_graph(dg, W.HAND_TIME, W.HAND_MAX_TIME, leave_out)
    view = dg.whole_graph(W.HAND_TIME, W.HAND_MAX_TIME, leave_out)
    assert len(view) == 7 and view.plan is None
    for got, want in zip(view[:5], a[:5]):
        assert isinstance(got, torch.Tensor) and not got.is_cuda and np.array_equal(got.numpy(), want)
    assert view[5] == a.node_dict and view[6] == a.edge_dict
    assert all(np.array_equal(x, y) for x, y in zip(view.sorted, a.sorted))
    assert view.type_rows("b") == slice(6, 11) and view.type_rows("c") == slice(11, 11)
    assert view.rows("d").tolist() == [11, 12, 13] and view.rows("b", [4, 0, 4]).tolist() == [10, 6, 10]
    assert dg.whole_graph()[2] is None


def test_missing_features_are_refused():
    csr = W.nested_to_csr(W.HAND_N, W.HAND_META, W.HAND_NESTED)
    feats = {t: np.zeros((n, 2), np.float32) for t, n in W.HAND_N.items()}
    with pytest.raises(ValueError):
        DeviceHeteroGraph.from_csr(W.HAND_TYPES, W.HAND_META, W.HAND_N, csr, dict(feats, b=None)).whole_graph()
    with pytest.raises(ValueError):
        DeviceHeteroGraph.from_csr(W.HAND_TYPES, W.HAND_META, W.HAND_N, csr, dict(feats, d=np.zeros((3, 5), np.float32))).whole_graph()
    with pytest.raises(ValueError):
        DeviceHeteroGraph.from_csr(W.HAND_TYPES, W.HAND_META, W.HAND_N, csr, None).whole_graph()
    assert np_whole_graph(DeviceHeteroGraph.from_csr(W.HAND_TYPES, W.HAND_META, W.HAND_N, csr, None)).node_feature is None


# ---------------------------------------------------------------------------------------------------- label_edge_flags
def test_label_edge_flags_equal_the_seed_mask_of_a_batch(small):
    """A sampled batch whose first seeds are `ids`, masked by seed_edge_mask: its edges are the unmasked batch's minus exactly those
    that label_edge_flags(ids) names -- the two helpers state one masking step (train_paper_field.py:109-122), one by serial, one by id"""
    _, dg = small
    ids, relations = [7, 2, 31, 12], ["AP_write", "rev_AP_write"]
    inp = {"paper": [[i, G.paper_year(i)] for i in ids + [20, 21]]}
    plain = sample_subgraph_host(dg, None, 2, G.SAMPLED_NUMBER, inp, seed=5)
    masked = sample_subgraph_host(dg, None, 2, G.SAMPLED_NUMBER, inp, seed=5, mask=seed_edge_mask(dg, relations, "paper", len(ids)))
    flags = label_edge_flags(dg, relations, "paper", ids)
    assert set(flags) == {("paper", "author", "AP_write"), ("author", "paper", "rev_AP_write")}
    assert flags[("paper", "author", "AP_write")][1] is None and flags[("author", "paper", "rev_AP_write")][0] is None
    assert np.flatnonzero(flags[("paper", "author", "AP_write")][0]).tolist() == sorted(ids)

    def rows(res, drop=None):
        orig = np.concatenate([res.indxs[t] for t in G.TYPES])
        ntype, ei, et = res[1].numpy(), res[3].numpy(), res[4].numpy()
        name = {v: k for k, v in dg.edge_dict.items()}
        out = []
        for e in range(ei.shape[1]):
            s, d = ei[0, e], ei[1, e]
            tri = (G.TYPES[ntype[d]], G.TYPES[ntype[s]], name[et[e]])
            tf, sf = (drop or {}).get(tri, (None, None))
            if (tf is not None and tf[orig[d]]) or (sf is not None and sf[orig[s]]):
                continue
            out.append((tri, int(orig[s]), int(orig[d])))
        return sorted(out)

    assert rows(masked) == rows(plain, flags) and len(rows(masked)) < len(rows(plain))
    # and on the whole graph: exactly the entries of those relations at those papers go
    full, cut = np_whole_graph(dg), np_whole_graph(dg, leave_out=flags)
    gone = full.edge_index.shape[1] - cut.edge_index.shape[1]
    ap = dg.csr[dg.triples.index(("paper", "author", "AP_write"))][0]
    assert gone == 2 * sum(int(ap[i + 1] - ap[i]) for i in ids)
    with pytest.raises(KeyError):
        label_edge_flags(dg, ["nope"], "paper", ids)
    with pytest.raises(IndexError):
        label_edge_flags(dg, relations, "paper", [40])
