"""CPU tests of the device sampler's definition (pyhgt_amd/sampler.py): the numpy sibling against the reference's sample_subgraph in
the regime where that draws no random number, the selection rule's distribution, the CSR builder and the argument rules of the C ABI;
the lists of whole calls that test_sampler_gpu.py compares with the sibling bit for bit, each certified here by the sibling's own
float64 keys, and the rows whose subset draw has a duplicated threshold word (tools/find_sampler_ties.py).  No kernel runs here."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest

from oracle.reference_loader import reference_available, load_reference_data
from pyhgt_amd import _lib
from pyhgt_amd.sampler import (DeviceHeteroGraph, sample_subgraph_host, sample_subgraph_device, philox4x32_10, np_select, np_select_keys,
                               np_budget_contributions, TIME_NONE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name="gen_golden_sampler"):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
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


# ---------------------------------------------------------------------------------------------------------------- whole calls
# The device draws the Philox words of the host sibling and holds the same integer scores, so a whole call can differ from the
# sibling's only where two fp32 selection keys order differently from their float64 twins.  A device key is within MARGIN = 1 + 2^-20
# of its float64 twin (test_sampler_gpu.py), two keys that move against each other need MARGIN ** 2, and the certificate asks for
# MARGIN ** 4 (a factor two of headroom in the exponent) between every pair of adjacent keys among the min(sampled_number + 1, n)
# smallest of every select step: then the chosen set and its serial order are those of the sibling, and by induction over the steps so
# is everything else.  The lists below are certified by the sibling alone, on the CPU; test_sampler_gpu.py runs them on the device.
MARGIN = 1.0 + 2.0 ** -20
CERTIFIED_GAP = MARGIN ** 4 - 1.0


def certificate_gap(trace, sampled_number):
    """smallest (ratio of adjacent keys - 1) among the min(sampled_number + 1, n) smallest float64 keys over the select steps of a
    trace of sample_subgraph_host; inf for a trace without two keys to compare"""
    gap = np.inf
    for _, _, ids, keys in trace:
        k = np.sort(keys)[:sampled_number + 1]
        if k.size > 1:
            gap = min(gap, float((k[1:] / k[:-1]).min() - 1.0))
    return gap


def host_certified(dg, call):
    """-> (result of the host sibling, certificate gap, number of select steps that had a candidate) of call = (inp, max_time, depth,
    sampled_number, seed)"""
    inp, max_time, depth, sn, seed = call
    trace = []
    res = sample_subgraph_host(dg, max_time, depth, sn, inp, seed, trace=trace)
    return res, certificate_gap(trace, sn), sum(1 for _, _, ids, _ in trace if ids.size)


OAG_TYPES = ["paper", "author", "field", "venue", "affiliation"]
OAG_N = {"paper": 6000, "author": 4000, "field": 45, "venue": 40, "affiliation": 200}
# (target, source, relation): venue rows (~600 papers) are above the hub line of 512, field rows (~530 +- 23) lie on both sides of it;
# paper <- venue carries no time; no triple has affiliation as its source, so nothing can ever be a candidate of that type
OAG_META = [("paper", "author", "AP_write"), ("author", "paper", "rev_AP_write"), ("paper", "venue", "PV"), ("venue", "paper", "rev_PV"),
            ("paper", "field", "PF"), ("field", "paper", "rev_PF"), ("paper", "paper", "PP_cite"), ("paper", "paper", "rev_PP_cite"),
            ("field", "field", "FF_in"), ("affiliation", "author", "AA_in")]


def oag_graph(device=None):
    from pyhgt_amd.synth import synthetic_hetero_csr
    csr = synthetic_hetero_csr(OAG_TYPES, OAG_META, OAG_N, mean_degree=4.0, seed=5, years=(-10, 10), none_time=("PV",))
    rng = np.random.default_rng(6)
    feats = {t: rng.standard_normal((OAG_N[t], 8)).astype(np.float32) for t in OAG_TYPES}
    return DeviceHeteroGraph.from_csr(OAG_TYPES, OAG_META, OAG_N, csr, feats, device=device)


def _ids(lo, n, stride, time):
    return [[lo + i * stride, time] for i in range(n)]


_PAPERS = {"paper": _ids(3, 32, 187, 4)}
_THREE = {"paper": _ids(1, 12, 499, 6), "author": _ids(2, 7, 571, -3), "venue": _ids(0, 3, 13, 0)}
_AFFIL = {"affiliation": _ids(5, 9, 21, 2)}                # a seed type nothing points into
# (seeds, max_time, depth, sampled_number, Philox seed)
OAG_CALLS = [(inp, max_time, depth, sn, seed) for inp, max_time, depth, sn, seeds in [
    (_PAPERS, 5, 0, 16, (0,)), (_THREE, None, 0, 128, (1,)),
    (_PAPERS, 5, 1, 1, (0, 1)), (_PAPERS, None, 1, 16, (2,)), (_THREE, 3, 1, 128, (3,)), (_AFFIL, None, 1, 128, (4,)),
    (_PAPERS, 5, 3, 16, (0, 1, 2, 3)), (_PAPERS, None, 3, 128, (5, 6)), (_THREE, -2, 3, 16, (7, 8)), (_THREE, None, 3, 1, (9, 10)),
    (_THREE, 3, 3, 128, (11, 16)), (_AFFIL, 4, 3, 16, (13, 14)), (_AFFIL, None, 3, 1, (15,))] for seed in seeds]


def _wide_meta(n_types, n_forward):
    types = ["t%02d" % i for i in range(n_types)]
    meta = []
    for i in range(n_forward):
        tt, st = types[i % n_types], types[(5 * i + 3) % n_types]
        meta += [(tt, st, "r%02d" % i), (st, tt, "rev_r%02d" % i)]
    return types, meta


def table_graph(kind, device=None):
    """the limits of the kernel-argument tables: `wide` = HGT_SAMPLER_MAX_TYPES types and HGT_SAMPLER_MAX_TRIPLES triples, ten to fifty
    nodes per type; `one` = one type, one triple (x, x, xx)"""
    from pyhgt_amd.synth import synthetic_hetero_csr
    if kind == "wide":
        types, meta = _wide_meta(_lib.HGT_SAMPLER_MAX_TYPES, _lib.HGT_SAMPLER_MAX_TRIPLES // 2)
        n = {t: 10 + (i * 7) % 41 for i, t in enumerate(types)}
    else:
        types, meta, n = ["x"], [("x", "x", "xx")], {"x": 300}
    csr = synthetic_hetero_csr(types, meta, n, mean_degree=5.0, seed=8, years=(-10, 10), none_time=("r03",))
    rng = np.random.default_rng(9)
    feats = {t: rng.standard_normal((n[t], 4)).astype(np.float32) for t in types}
    return DeviceHeteroGraph.from_csr(types, meta, n, csr, feats, device=device)


TABLE_CALLS = {"wide": [({"t00": _ids(0, 4, 2, 3), "t07": _ids(1, 3, 3, -1), "t15": _ids(0, 2, 5, 8)}, 6, 3, 4, 0),
                        ({"t05": _ids(0, 5, 2, 0)}, None, 2, 16, 1)],
               "one": [({"x": _ids(2, 6, 31, 1)}, 5, 3, 4, 0), ({"x": _ids(0, 3, 100, -4)}, None, 2, 16, 1)]}


@pytest.fixture(scope="module")
def oag():
    return oag_graph()


def test_trace_hook_reports_every_select_step(oag):
    """the trace of a call: one entry per (layer, type) in step order, and re-ranking its keys gives the nodes the call added"""
    inp, max_time, depth, sn, seed = next(c for c in OAG_CALLS if c[0] is _AFFIL and c[2] == 3 and c[3] == 16)
    trace = []
    res = sample_subgraph_host(oag, max_time, depth, sn, inp, seed, trace=trace)
    plain = sample_subgraph_host(oag, max_time, depth, sn, inp, seed)
    assert all(np.array_equal(a, b) for a, b in zip(res.sorted, plain.sorted))
    T = len(OAG_TYPES)
    assert [(t, step) for t, step, _, _ in trace] == [(t, T * (1 + layer) + t) for layer in range(depth) for t in range(T)]
    taken = {t: len(inp.get(t, [])) for t in OAG_TYPES}
    for t, step, ids, keys in trace:
        assert ids.dtype == np.int64 and keys.dtype == np.float64 and ids.shape == keys.shape and np.all(keys > 0)
        new = ids[np.lexsort((ids, keys))[:sn]]
        name = OAG_TYPES[t]
        assert np.array_equal(res.indxs[name][taken[name]:taken[name] + new.size], new), (name, step)
        taken[name] += new.size
    assert taken == {t: len(res.indxs[t]) for t in OAG_TYPES}
    assert not any(ids.size for t, _, ids, _ in trace if OAG_TYPES[t] == "affiliation") and len(res.indxs["affiliation"]) == 9


def test_whole_call_lists_are_certified(oag):
    """every call the GPU tests compare whole is certified by the host sibling alone; the lists cover depth 0 / 1 / 3, sampled_number
    1 / 16 / 128, max_time set and None, one and three seed types and a seed type nothing points into"""
    assert len(OAG_CALLS) >= 16 and {c[2] for c in OAG_CALLS} == {0, 1, 3} and {c[3] for c in OAG_CALLS} == {1, 16, 128}
    assert {c[1] is None for c in OAG_CALLS} == {True, False} and {len(c[0]) for c in OAG_CALLS} == {1, 3}
    hubs = [int((np.diff(ip) > 512).sum()) for ip, _, _ in oag.csr]
    rows = sum(ip.size - 1 for ip, _, _ in oag.csr)
    assert sum(1 for h in hubs if h) >= 2 and sum(hubs) < rows // 50, hubs
    smallest, drew = np.inf, 0
    for graph, calls in [(oag, OAG_CALLS)] + [(table_graph(k), TABLE_CALLS[k]) for k in ("wide", "one")]:
        for i, call in enumerate(calls):
            res, gap, steps = host_certified(graph, call)
            assert gap > CERTIFIED_GAP, "call %d of %s: gap %.3g" % (i, graph.types[:2], gap)
            assert call[2] == 0 or steps > 0
            smallest, drew = min(smallest, gap), drew + steps
    print("smallest certified gap %.3g (threshold %.3g) over %d select steps" % (smallest, CERTIFIED_GAP, drew))
    wide = table_graph("wide")
    assert len(wide.types) == _lib.HGT_SAMPLER_MAX_TYPES and len(wide.triples) == _lib.HGT_SAMPLER_MAX_TRIPLES
    assert all(10 <= n <= 50 for n in wide.n_nodes)


# ---------------------------------------------------------------------------------------------------------------- ties of the subset draw
# Found by tools/find_sampler_ties.py (its defaults, 2.9 s; --degree 512 --targets 4096 --seeds 64, 4.5 s): rows whose r-th and
# (r + 1)-th smallest Philox words are equal.  seed, target id, step, triple index, degree, r, the word, its two positions.
TIES = {"workgroup": dict(seed=0, target=119, step=0, triple=0, degree=60000, r=486, word=0x02110750, positions=(32474, 49873)),
        "wavefront": dict(seed=2, target=1360, step=0, triple=0, degree=512, r=248, word=0x829cb37c, positions=(203, 255))}
TIE_N = {"x": 1400, "y": 60000}


def tie_graph(device=None):
    """x <- y, one triple: the two rows of TIES (each neighbour list a permutation prefix of y, so the tied positions hold different
    ids), every other row empty"""
    rng = np.random.default_rng(14)
    deg = np.zeros(TIE_N["x"], np.int64)
    for tie in TIES.values():
        deg[tie["target"]] = tie["degree"]
    indptr = np.concatenate([[0], np.cumsum(deg)])
    src = np.concatenate([rng.permutation(TIE_N["y"])[:d] for d in deg[deg > 0]])
    tm = rng.integers(-10, 10, size=src.size)
    tm[rng.random(src.size) < 0.1] = TIME_NONE
    feats = {t: np.zeros((n, 1), np.float32) for t, n in TIE_N.items()}
    return DeviceHeteroGraph.from_csr(["x", "y"], [("x", "y", "xy")], TIE_N, [(indptr, src, tm)], feats, device=device)


@pytest.mark.parametrize("name", list(TIES))
def test_tie_fixtures_sit_where_the_constants_say(name):
    tie = TIES[name]
    F = _tool("find_sampler_ties")
    words = F.row_words(tie["degree"], tie["target"], tie["step"], tie["triple"], tie["seed"])
    order = np.lexsort((np.arange(words.size), words))
    r = tie["r"]
    assert 1 <= r and r + 1 < tie["degree"] and r + 1 <= _lib.HGT_SAMPLER_MAX_NUMBER          # sampled_number = r and r + 1 both draw
    assert (name == "wavefront") == (tie["degree"] <= _lib.HGT_SAMPLER_HUB_DEG)
    assert words[order[r - 1]] == words[order[r]] == tie["word"] and (order[r - 1], order[r]) == tie["positions"]
    assert words[order[r - 2]] < tie["word"] < words[order[r + 1]]                            # a tie of exactly two
    assert F.tie_of_row(words, r) == (r, tie["word"]) + tie["positions"]
    dg = tie_graph()
    indptr, src, tm = dg.csr[tie["triple"]]
    beg = indptr[tie["target"]]
    assert indptr[tie["target"] + 1] - beg == tie["degree"]
    p, q = tie["positions"]
    assert src[beg + p] != src[beg + q]
    # breaking the tie the other way changes the result: both neighbours pass the filters of the draw the GPU test makes
    s, add, _ = np_budget_contributions(dg.csr[0], 0, [tie["target"]], [0], tie["step"], r, None, tie["seed"], np.full(TIE_N["y"], -1))
    assert s.size == r and src[beg + p] in s and src[beg + q] not in s
