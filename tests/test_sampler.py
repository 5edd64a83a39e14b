"""CPU tests of the device sampler's definition (pyhgt_amd/sampler.py): the numpy sibling against the reference's sample_subgraph in
the regime where that draws no random number, the selection rule's distribution, the CSR builder and the argument rules of the C ABI.
No kernel runs here."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest

from oracle.reference_loader import reference_available, load_reference_data
from pyhgt_amd import _lib
from pyhgt_amd.sampler import (DeviceHeteroGraph, sample_subgraph_host, sample_subgraph_device, philox4x32_10, np_select, np_select_keys,
                               TIME_NONE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("gen_golden_sampler", os.path.join(ROOT, "tools", "gen_golden_sampler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _tool()


@pytest.fixture(scope="module")
def small():
    edges = G.synthetic_edges()
    feats = {t: np.arange(G.N_NODES[t], dtype=np.float32).reshape(-1, 1) for t in G.TYPES}
    return edges, DeviceHeteroGraph.from_csr(G.TYPES, G.META, G.N_NODES, G.csr_from_edges(edges), feats), np.load(G.GOLDEN)


def _canonical(res):
    return G.canonical(G.TYPES, res.indxs, res.times, res[3].numpy(), res[4].numpy(), res[2].numpy(), res[5])


def test_philox_known_answers():
    """Random123's known-answer vectors of philox4x32_10"""
    kat = [((0, 0, 0, 0), 0, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, 0xffffffffffffffff, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0x299f31d0 << 32) | 0xa4093822, (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert tuple(int(w) for w in philox4x32_10(*ctr, key)) == out


@pytest.mark.parametrize("case", list(G.CASES))
def test_deterministic_regime_equals_the_fixtures(small, case):
    """sampled_number above every degree and budget size: node sets, times, edges per relation and edge times of the committed
    reference output, after relabelling by original id.  Cases: None times (paper <- venue), papers newer than max_time, an empty
    type, depth 0, no time filter, seeds of two types."""
    _, dg, fx = small
    inp, max_time, depth = G.CASES[case]
    res = sample_subgraph_host(dg, max_time, depth, G.SAMPLED_NUMBER, inp, seed=3)
    nodes, rows = _canonical(res)
    for t in G.TYPES:
        assert np.array_equal(nodes[t], fx["%s/nodes/%s" % (case, t)]), t
    assert np.array_equal(rows, fx["%s/edges" % case])
    # the layout: type-contiguous nodes, relation-major edges with non-decreasing targets, the feature rows of the sampled ids
    src, dst, etime, rel_ptr, type_off = res.sorted
    assert rel_ptr[0] == 0 and rel_ptr[-1] == src.size and type_off[-1] == res[1].numel()
    for r in range(len(rel_ptr) - 1):
        assert np.all(np.diff(dst[rel_ptr[r]:rel_ptr[r + 1]]) >= 0)
    assert np.array_equal(res[0].numpy()[:, 0], np.concatenate([res.indxs[t] for t in G.TYPES]).astype(np.float32))
    if case == "depth2":      # the cases are not trivial: a filtered paper, an inherited time
        assert 4 not in nodes["paper"][:, 0] % 5 and len(nodes["venue"]) == 4 and len(nodes["empty"]) == 0
        assert np.array_equal(nodes["venue"][:, 1], 2000 + nodes["venue"][:, 0])


@pytest.mark.skipif(not reference_available(), reason="the reference tree is not present")
@pytest.mark.parametrize("case", list(G.CASES))
def test_deterministic_regime_equals_the_live_reference(small, case):
    edges, dg, fx = small
    data = load_reference_data()
    nodes_ref, rows_ref = G.run_reference(data, G.reference_graph(data, edges), case)
    inp, max_time, depth = G.CASES[case]
    nodes, rows = _canonical(sample_subgraph_host(dg, max_time, depth, G.SAMPLED_NUMBER, inp, seed=11))
    for t in G.TYPES:
        assert np.array_equal(nodes[t], nodes_ref[t]) and np.array_equal(nodes_ref[t], fx["%s/nodes/%s" % (case, t)])
    assert np.array_equal(rows, rows_ref) and np.array_equal(rows_ref, fx["%s/edges" % case])


def _inclusion_probabilities(w, k):
    """exact inclusion probabilities of successive weighted sampling of k items without replacement"""
    n, p = len(w), np.zeros(len(w))
    for perm in itertools.permutations(range(n), k):
        rest, pr = float(np.sum(w)), 1.0
        for i in perm:
            pr *= w[i] / rest
            rest -= w[i]
        p[list(perm)] += pr
    return p


def test_selection_follows_successive_weighted_sampling():
    """8 candidates with unequal scores, k = 3, 4096 fixed seeds: inclusion frequencies of the exponential-key rule against the exact
    probabilities of drawing with p = score^2 / sum without replacement (data.py:161-163), each within 5 standard deviations; the same
    check on np.random.choice shows that the yardstick is the reference's distribution."""
    terms = np.array([1, 2, 3, 4, 6, 8, 12, 16], dtype=np.uint64)
    ids = np.array([5, 17, 2, 40, 33, 8, 21, 11])
    score = np.zeros(64, np.uint64)
    score[ids] = terms * np.uint64(2 ** 32 // 16)
    w = (score[ids].astype(np.float64) * 2.0 ** -32) ** 2
    p = _inclusion_probabilities(w, 3)
    assert abs(p.sum() - 3) < 1e-12 and p.max() < 0.95 and p.min() > 0.005
    n, bound = 4096, 5 * np.sqrt(p * (1 - p) / 4096)
    ours, theirs = np.zeros(8), np.zeros(8)
    pos = {v: i for i, v in enumerate(ids)}
    rs = np.random.RandomState(0)
    for seed in range(n):
        chosen = np_select(ids, score, 1, 9, seed, 3)
        assert len(set(chosen.tolist())) == 3
        ours[[pos[v] for v in chosen]] += 1
        theirs[rs.choice(8, 3, p=w / w.sum(), replace=False)] += 1
    print("p", p.round(4), "ours", (ours / n).round(4), "np.random.choice", (theirs / n).round(4))
    assert np.all(np.abs(ours / n - p) <= bound), (ours / n - p) / bound
    assert np.all(np.abs(theirs / n - p) <= bound), (theirs / n - p) / bound
    # the serial order is the key order, ties to the smaller id
    keys = np_select_keys(ids, score, 1, 9, 0)
    assert np.array_equal(np_select(ids, score, 1, 9, 0, 8), ids[np.lexsort((ids, keys))])


class _FakeGraph:
    def __init__(self, types, edge_list):
        self._types, self.edge_list = types, edge_list

    def get_types(self):
        return list(self._types)


def test_csr_builder_round_trip():
    """graph.edge_list -> CSRs: neighbours keep the dict's order, None times become TIME_NONE, a `self` relation is ignored"""
    el = {"a": {"b": {"ab": {2: {1: 2001, 0: None}, 0: {2: 1999}}, "self": {0: {0: None}}}}, "b": {"a": {"rev_ab": {1: {2: 2001}, 0: {2: None}, 2: {0: 1999}}}}}
    feats = {"a": np.zeros((3, 2), np.float32), "b": np.ones((3, 2), np.float32), "c": None}
    dg = DeviceHeteroGraph.from_reference_graph(_FakeGraph(["a", "b", "c"], el), feats)
    assert dg.get_meta_graph() == [("a", "b", "ab"), ("b", "a", "rev_ab")] and dg.n_nodes == [3, 3, 0]
    assert dg.edge_dict == {"ab": 0, "rev_ab": 1, "self": 2}
    ip, src, tm = dg.csr[0]
    assert ip.tolist() == [0, 1, 1, 3] and src.tolist() == [2, 1, 0] and tm.tolist() == [1999, 2001, TIME_NONE]
    ip, src, tm = dg.csr[1]
    assert ip.tolist() == [0, 1, 2, 3] and src.tolist() == [2, 2, 0] and tm.tolist() == [TIME_NONE, 2001, 1999]
    # from_csr with the same arrays gives the same graph; the sampler walks it
    dg2 = DeviceHeteroGraph.from_csr(["a", "b", "c"], dg.get_meta_graph(), {"a": 3, "b": 3, "c": 0}, dg.csr, feats)
    res = sample_subgraph_host(dg2, 2001, 1, 4, {"a": [[2, 2001]]}, seed=0)
    assert sorted(res.indxs["b"].tolist()) == [0, 1] and res.indxs["a"].tolist() == [2]
    assert dict(zip(res.indxs["b"].tolist(), res.times["b"].tolist())) == {1: 2001, 0: 2001}      # None inherits the target's time
    with pytest.raises(ValueError):
        DeviceHeteroGraph.from_csr(["a", "b"], [("a", "b", "ab")], {"a": 3, "b": 3}, [(np.array([0, 1, 1, 3]), np.array([2, 1, 5]), None)])
    with pytest.raises(ValueError):
        DeviceHeteroGraph.from_csr(["a", "b"], [("a", "b", "ab")], {"a": 3, "b": 3}, [(np.array([0, 1, 3]), np.array([2, 1, 0]), None)])


def test_host_sampler_random_regime_is_valid_and_repeatable(small):
    _, dg, _ = small
    inp = {"paper": [[0, 2000], [1, 2001]]}
    a = sample_subgraph_host(dg, 2003, 2, 3, inp, seed=21)
    b = sample_subgraph_host(dg, 2003, 2, 3, inp, seed=21)
    c = sample_subgraph_host(dg, 2003, 2, 3, inp, seed=22)
    assert all(np.array_equal(x, y) for x, y in zip(a.sorted, b.sorted)) and all(np.array_equal(a.indxs[t], b.indxs[t]) for t in G.TYPES)
    assert any(not np.array_equal(a.indxs[t], c.indxs[t]) for t in G.TYPES)
    assert len(a.indxs["paper"]) == 2 + 2 * 3 and len(a.indxs["venue"]) <= 2 * 3 and len(a.indxs["empty"]) == 0
    for t in G.TYPES:
        assert len(set(a.indxs[t].tolist())) == len(a.indxs[t])
    # the state arrays are clean again: a deterministic call after the random ones still equals the fixture
    nodes, _ = _canonical(sample_subgraph_host(dg, 2003, 2, G.SAMPLED_NUMBER, G.CASES["depth2"][0], seed=0))
    assert np.array_equal(nodes["paper"], small[2]["depth2/nodes/paper"])


def test_device_sampler_refuses_a_host_graph(small):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sample_subgraph_device(small[1], 2003, 1, 4, {"paper": [[0, 2000]]}, seed=0)
    with pytest.raises(ValueError):
        sample_subgraph_host(small[1], 2003, 1, _lib.HGT_SAMPLER_MAX_NUMBER + 1, {"paper": [[0, 2000]]}, seed=0)
    with pytest.raises(ValueError):
        sample_subgraph_host(small[1], 2003, 1, 4, {"paper": [[0, 2000], [0, 2001]]}, seed=0)
    with pytest.raises(IndexError):
        sample_subgraph_host(small[1], 2003, 1, 4, {"paper": [[40, 2000]]}, seed=0)


def _tables(n_nodes=8, cap_s=4, cap_c=8):
    """type / triple tables over host buffers: every call below must return before it launches anything"""
    buf = (C.c_uint64 * 64)()
    p = C.addressof(buf)
    types = (_lib.HgtSamplerType * 2)()
    for t in range(2):
        types[t] = _lib.HgtSamplerType(p, p, p, p, p, p, n_nodes, cap_s, cap_c, 0)
    triples = (_lib.HgtSamplerTriple * 2)()
    triples[0] = _lib.HgtSamplerTriple(p, p, p, 0, 1, 0, 0)
    triples[1] = _lib.HgtSamplerTriple(p, p, p, 1, 0, 1, 0)
    return buf, p, types, triples


def test_sampler_abi_argument_rules():
    lib = _lib.load()
    buf, p, types, triples = _tables()
    INV, UNS, WS = -1, -2, -3
    slots = C.c_int64()
    assert lib.hgt_sampler_induce_slots(types, 2, triples, 2, C.byref(slots)) == 0 and slots.value == 8
    assert lib.hgt_sampler_induce_slots(types, 2, triples, 2, None) == INV
    # tables: NULL, sizes out of range, more entries than the limits
    assert lib.hgt_sampler_seed(None, 2, 0, p, p, 2, 0, None) == INV
    assert lib.hgt_sampler_seed(types, 0, 0, p, p, 2, 0, None) == INV
    assert lib.hgt_sampler_seed(types, _lib.HGT_SAMPLER_MAX_TYPES + 1, 0, p, p, 2, 0, None) == UNS
    assert lib.hgt_sampler_add_budget(types, 2, triples, _lib.HGT_SAMPLER_MAX_TRIPLES + 1, 0, 0, 4, 2, 0, 0, 1, p, 64, None) == UNS
    assert lib.hgt_sampler_add_budget(types, 2, None, 2, 0, 0, 4, 2, 0, 0, 1, p, 64, None) == INV
    assert lib.hgt_sampler_reset(None, 2, None) == INV
    bad = _tables(cap_s=9)[2]                                # a list longer than the type has nodes
    assert lib.hgt_sampler_reset(bad, 2, None) == INV
    bad = _tables()[2]
    bad[1].counts = None
    assert lib.hgt_sampler_reset(bad, 2, None) == INV
    bad = _tables()[3]
    bad[1].src_type = 2
    assert lib.hgt_sampler_add_budget(types, 2, bad, 2, 0, 0, 4, 2, 0, 0, 1, p, 64, None) == INV
    # seed: type, count, arrays, capacity
    assert lib.hgt_sampler_seed(types, 2, 2, p, p, 2, 0, None) == INV
    assert lib.hgt_sampler_seed(types, 2, 0, p, p, -1, 0, None) == INV
    assert lib.hgt_sampler_seed(types, 2, 0, None, p, 2, 0, None) == INV
    assert lib.hgt_sampler_seed(types, 2, 0, p, p, 5, 0, None) == WS
    # add_budget: sampled_number, negative sizes, scratch
    assert lib.hgt_sampler_add_budget(types, 2, triples, 2, 0, 0, 0, 2, 0, 0, 1, p, 64, None) == INV
    assert lib.hgt_sampler_add_budget(types, 2, triples, 2, 0, 0, _lib.HGT_SAMPLER_MAX_NUMBER + 1, 2, 0, 0, 1, p, 64, None) == UNS
    assert lib.hgt_sampler_add_budget(types, 2, triples, 2, 0, -1, 4, 2, 0, 0, 1, p, 64, None) == INV
    assert lib.hgt_sampler_add_budget(types, 2, triples, 2, 0, 0, 4, -2, 0, 0, 1, p, 64, None) == INV
    assert lib.hgt_sampler_add_budget(types, 2, triples, 2, 0, 0, 4, 2, 0, 0, 1, None, 64, None) == INV
    assert lib.hgt_sampler_add_budget(types, 2, triples, 2, 0, 0, 4, 2, 0, 0, 1, p, 2, None) == WS
    assert lib.hgt_sampler_add_budget(types, 2, triples, 2, 0, 0, 4, 0, 0, 0, 1, None, 0, None) == 0      # no row: nothing to do
    # select
    assert lib.hgt_sampler_select(types, 2, 0, 0, 4, 1, None, p, 8, None) == INV
    assert lib.hgt_sampler_select(types, 2, 0, 0, 4, 1, p, p, 7, None) == WS
    assert lib.hgt_sampler_select(types, 2, 0, 0, _lib.HGT_SAMPLER_MAX_NUMBER + 1, 1, p, p, 8, None) == UNS
    assert lib.hgt_sampler_select(types, 2, -1, 0, 4, 1, p, p, 8, None) == INV
    # induce: relation ids in order and below `self`, scratch, sizes
    assert lib.hgt_sampler_induce_count(types, 2, triples, 2, 3, p, p, 8, p, p, p, None) == WS
    assert lib.hgt_sampler_induce_count(types, 2, triples, 2, 2, p, p, 9, p, p, p, None) == INV      # rel_id 1 is not below self = 1
    assert lib.hgt_sampler_induce_count(types, 2, triples, 2, 3, None, p, 9, p, p, p, None) == INV
    swapped = _tables()[3]
    swapped[0].rel_id, swapped[1].rel_id = 1, 0
    assert lib.hgt_sampler_induce_count(types, 2, swapped, 2, 3, p, p, 9, p, p, p, None) == INV
    assert lib.hgt_sampler_induce_fill(types, 2, triples, 2, 3, p, p, 9, p, 4, 3, p, p, p, p, p, None) == INV      # fewer edges than self loops
    assert lib.hgt_sampler_induce_fill(types, 2, triples, 2, 3, p, p, 9, p, -1, 3, p, p, p, p, p, None) == INV
    assert lib.hgt_sampler_induce_fill(types, 2, triples, 2, 3, p, p, 9, p, 4, 6, None, p, p, p, p, None) == INV
    assert lib.hgt_sampler_induce_fill(types, 2, triples, 2, 3, p, p, 8, p, 4, 6, p, p, p, p, p, None) == WS
    assert lib.hgt_sampler_induce_fill(types, 2, triples, 2, 3, p, p, 9, p, 4, 2 ** 31, p, p, p, p, p, None) == -4
    del buf
