"""CPU tests of the graph build's definition (pyhgt_amd/graph_build.py): `np_edge_lists_to_csr` against a literal restatement of
ogbn-mag/preprocess_ogbn_mag.py:29-42 (nested defaultdicts, one step per edge) read by the existing `from_reference_graph`;
`.degree` against the script's line 63; `np_neighbour_mean` against lines 81-86 with a dense count matrix; the host sampler on both
graphs; every documented error.  No kernel runs here; test_graph_build_gpu.py compares the device build with this definition."""
from collections import OrderedDict, defaultdict

import numpy as np
import pytest
import torch

from pyhgt_amd import DeviceHeteroGraph, np_edge_lists_to_csr, np_neighbour_mean, sample_subgraph_host
from pyhgt_amd.sampler import TIME_NONE

TYPES = ["paper", "author", "field", "institution", "venue"]           # `venue` has no relation at all


class StubGraph:
    """what from_reference_graph reads of the reference's Graph"""

    def __init__(self, types):
        self._types = list(types)
        self.edge_list = defaultdict(lambda: defaultdict(lambda: defaultdict(lambda: defaultdict(dict))))

    def get_types(self):
        return list(self._types)


def script_graph(types, edges, edge_time=None, node_time=None, reverse="rev_"):
    """preprocess_ogbn_mag.py:29-42, with `'paper'` read as "a type that has a node_time table" and the per-edge times of other
    datasets in front of it; reverse=None leaves line 42 out"""
    edge_time, node_time = edge_time or {}, node_time or {}
    graph = StubGraph(types)
    edg = graph.edge_list
    for key in edges:
        ei = edges[key]
        ei = ei.cpu().numpy() if isinstance(ei, torch.Tensor) else np.asarray(ei)
        s_type, r_type, t_type = key
        elist = edg[t_type][s_type][r_type]
        rlist = edg[s_type][t_type][reverse + r_type] if reverse is not None else None
        for e, (s_id, t_id) in enumerate(ei.T.tolist()):
            year = None
            if key in edge_time:
                year = int(edge_time[key][e])
                year = None if year == TIME_NONE else year
            elif s_type in node_time:
                year = int(node_time[s_type][s_id])
            elif t_type in node_time:
                year = int(node_time[t_type][t_id])
            elist[t_id][s_id] = year
            if rlist is not None:
                rlist[s_id][t_id] = year
    return graph


def script_degree(graph, n_nodes):
    """lines 46-63"""
    deg = {key: np.zeros(n_nodes[key]) for key in n_nodes}
    for k1 in graph.edge_list:
        for k2 in graph.edge_list[k1]:
            for k3 in graph.edge_list[k1][k2]:
                for e1 in graph.edge_list[k1][k2][k3]:
                    if len(graph.edge_list[k1][k2][k3][e1]) == 0:
                        continue
                    deg[k1][e1] += len(graph.edge_list[k1][k2][k3][e1])
    return deg


def features(n_nodes, width=3):
    return {t: (np.arange(n * width, dtype=np.float32).reshape(n, width) * 0.5 + i) for i, (t, n) in enumerate(n_nodes.items())}


def raw_relations(E, seed, n_nodes=None, dtype=np.int64, repeat_share=0.25):
    """four MAG-shaped relations of E edges each over a few nodes, so that pairs repeat by themselves; a share of the later edges are
    copies of earlier ones (far apart when E is large); the upper half of every type's ids is never used (rows of length 0)"""
    rng = np.random.default_rng(seed)
    n_nodes = n_nodes or {"paper": 40, "author": 31, "field": 7, "institution": 3, "venue": 5}
    keys = [("author", "affiliated_with", "institution"), ("author", "writes", "paper"), ("paper", "cites", "paper"),
            ("paper", "has_topic", "field")]
    edges = OrderedDict()
    for key in keys:
        hi_s, hi_t = max(1, (n_nodes[key[0]] + 1) // 2), max(1, (n_nodes[key[2]] + 1) // 2)
        ei = np.stack([rng.integers(0, hi_s, E), rng.integers(0, hi_t, E)]).astype(dtype)
        for e in range(E):
            if e and rng.random() < repeat_share:
                ei[:, e] = ei[:, rng.integers(0, max(1, e // 4))]
        edges[key] = ei
    return n_nodes, edges


def times_for(edges, n_nodes, seed, missing=True):
    """per-edge times that differ between the copies of a pair, some of them missing, and a year per node of every type"""
    rng = np.random.default_rng(seed + 1000)
    edge_time = {}
    for key, ei in edges.items():
        tm = rng.integers(1990, 2020, ei.shape[1]).astype(np.int32)
        if missing:
            tm[rng.random(ei.shape[1]) < 0.2] = TIME_NONE
        edge_time[key] = tm
    node_time = {t: rng.integers(1990, 2020, n).astype(np.int32) for t, n in n_nodes.items()}
    return edge_time, node_time


def assert_same_graph(got, want):
    assert got.types == want.types and got.n_nodes == want.n_nodes
    assert got.meta == want.meta, "meta in the dicts' insertion order"
    assert got.triples == want.triples and got.tri_types == want.tri_types and got.edge_dict == want.edge_dict
    assert len(got.csr) == len(want.csr) == len(want.triples)
    for tri, a, b in zip(want.triples, got.csr, want.csr):
        for x, y, name in zip(a, b, ("indptr", "src", "time")):
            assert x.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), (tri, name)


# node_time on: the source side and the target side and neither (paper), both sides (paper + author), per-edge times, no times
TIME_CASES = OrderedDict([
    ("paper_years", lambda et, nt: (None, {"paper": nt["paper"]})),
    ("paper_and_author_years", lambda et, nt: (None, {"paper": nt["paper"], "author": nt["author"]})),
    ("field_years_only", lambda et, nt: (None, {"field": nt["field"]})),
    ("edge_times", lambda et, nt: (et, None)),
    ("edge_times_and_institution_years", lambda et, nt: ({k: v for k, v in et.items() if k[1] in ("cites", "has_topic")}, {"institution": nt["institution"]})),
    ("no_times", lambda et, nt: (None, None)),
])


@pytest.mark.parametrize("reverse", ["rev_", None, "back_"])
@pytest.mark.parametrize("case", list(TIME_CASES))
@pytest.mark.parametrize("E", [0, 1, 90, 700])
def test_rule_equals_the_scripts_dicts(E, case, reverse):
    n_nodes, edges = raw_relations(E, seed=E + 3)
    et, nt = TIME_CASES[case](*times_for(edges, n_nodes, E))
    want = DeviceHeteroGraph.from_reference_graph(script_graph(TYPES, edges, et, nt, reverse), None, n_nodes=n_nodes)
    meta, csr = np_edge_lists_to_csr(TYPES, n_nodes, edges, et, nt, reverse)
    assert meta == want.meta
    got = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, edges, et, nt, reverse=reverse)
    assert_same_graph(got, want)
    assert len(want.meta) == (4 if reverse is None else 8)
    if reverse is None:                                                  # author is only ever a source: nothing points into it
        assert not any(tt == "author" for tt, _, _ in got.triples)
    if E == 700:                                                         # the inputs are not trivial
        ip, src, tm = got.csr[got.triples.index(("paper", "paper", "cites"))]
        assert src.size < E and (np.diff(ip) == 0).sum() >= n_nodes["paper"] // 2 and np.diff(ip).max() > 8
        if case == "edge_times":
            assert (tm == TIME_NONE).any() and (tm != TIME_NONE).any()
    # line 63, after the repeats are gone
    deg = script_degree(script_graph(TYPES, edges, et, nt, reverse), n_nodes)
    for t in TYPES:
        assert got.degree[t].dtype == np.int32 and np.array_equal(got.degree[t], deg[t]), t
        assert np.array_equal(want.degree[t], deg[t])                    # a graph built the old way answers too


def test_first_position_last_time_far_apart():
    """the pair (target 2, source 5) at entries 0, 1 (adjacent), 2500 and 4999 with four times: it stays the first neighbour of its
    row and carries the last time; a row made of one repeated pair; a self-typed relation whose reverse lands on the same type pair"""
    E = 5000
    rng = np.random.default_rng(5)
    ei = np.stack([rng.integers(0, 50, E), rng.integers(3, 60, E)])
    tm = rng.integers(0, 100, E).astype(np.int32)
    for e, year in ((0, 11), (1, 12), (2500, 13), (4999, 14)):
        ei[:, e], tm[e] = (5, 2), year
    ei[:, 100:140] = np.array([[7], [0]])                                 # row 0: forty copies of one pair
    tm[100:140] = np.arange(40)
    n_nodes = {"paper": 64}
    edges = {("paper", "cites", "paper"): ei}
    got = DeviceHeteroGraph.from_edge_lists(["paper"], n_nodes, edges, {("paper", "cites", "paper"): tm})
    want = DeviceHeteroGraph.from_reference_graph(script_graph(["paper"], edges, {("paper", "cites", "paper"): tm}), None, n_nodes=n_nodes)
    assert_same_graph(got, want)
    assert got.triples == [("paper", "paper", "cites"), ("paper", "paper", "rev_cites")]
    ip, src, t = got.csr[0]
    assert src[ip[2]] == 5 and t[ip[2]] == 14
    assert ip[1] - ip[0] == 1 and src[ip[0]] == 7 and t[ip[0]] == 39
    ip, src, t = got.csr[1]                                               # the reverse: row 5 starts with 2, row 7 holds 0
    assert src[ip[5]] == 2 and t[ip[5]] == 14 and 0 in src[ip[7]:ip[8]]


def test_inputs_of_any_kind_give_the_same_graph():
    n_nodes, edges = raw_relations(300, seed=8)
    et, nt = times_for(edges, n_nodes, 8)
    want = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, edges, None, {"paper": nt["paper"]})
    kinds = {
        "int32": lambda a: a.astype(np.int32),
        "transposed view": lambda a: np.ascontiguousarray(a.T).T,
        "torch": lambda a: torch.from_numpy(a),
        "torch .t() view": lambda a: torch.from_numpy(a).t().contiguous().t(),
    }
    for name, conv in kinds.items():
        got = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, OrderedDict((k, conv(v)) for k, v in edges.items()), None,
                                                {"paper": torch.from_numpy(nt["paper"])})
        assert_same_graph(got, want)


@pytest.mark.parametrize("seed", [1, 2])
def test_host_sampler_draws_the_same_batches(seed):
    """the random words are keyed by triple index and neighbour position: identical CSRs, identical batches"""
    n_nodes, edges = raw_relations(900, seed=seed, n_nodes={"paper": 120, "author": 90, "field": 20, "institution": 6, "venue": 2})
    _, nt = times_for(edges, n_nodes, seed)
    feats = features(n_nodes)
    a = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, edges, node_time={"paper": nt["paper"]}, features=feats)
    b = DeviceHeteroGraph.from_reference_graph(script_graph(TYPES, edges, None, {"paper": nt["paper"]}), feats)
    inp = {"paper": [[i, 2015] for i in range(8)]}
    ra, rb = (sample_subgraph_host(g, 2015, 2, 4, inp, seed=7 + seed) for g in (a, b))      # sampled_number 4: rows draw
    for x, y in zip(ra.sorted, rb.sorted):
        assert np.array_equal(x, y)
    for t in TYPES:
        assert np.array_equal(ra.indxs[t], rb.indxs[t]) and np.array_equal(ra.times[t], rb.times[t])
    assert torch.equal(ra[0], rb[0]) and ra[0].shape[0] > 20


def test_neighbour_mean_rule_equals_the_scripts_matrix_product():
    """lines 81-86 without scipy: a dense [n_t, n_s] count matrix (coo_matrix sums what two relations share), normalize, dot"""
    n_nodes = {"paper": 40, "author": 31, "field": 7, "institution": 3, "venue": 5}
    rng = np.random.default_rng(4)
    ei1 = np.stack([rng.integers(0, 40, 200), rng.integers(0, 20, 200)])
    ei2 = np.concatenate([ei1[:, :30], np.stack([rng.integers(0, 40, 50), rng.integers(0, 20, 50)])], axis=1)
    edges = OrderedDict([(("paper", "written_by", "author"), ei1), (("paper", "reviewed_by", "author"), ei2)])
    g = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, edges)
    x = rng.uniform(-1e4, 1e4, (40, 6))
    count = np.zeros((31, 40))
    for m, (tt, st, _) in enumerate(g.triples):
        if (tt, st) == ("author", "paper"):
            ip, src, _ = g.csr[m]
            np.add.at(count, (np.repeat(np.arange(31), np.diff(ip)), src), 1.0)
    assert count.max() == 2.0 and (count.sum(1) == 0).any()
    rowsum = count.sum(1)
    r_inv = np.where(rowsum > 0, 1.0 / np.maximum(rowsum, 1), 0.0)       # normalize: the infinite reciprocal becomes 0
    want = (count * r_inv[:, None]) @ x
    got = np_neighbour_mean(g, "author", "paper", x)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12, atol=1e-9)
    assert np.array_equal(got[rowsum == 0], np.zeros(((rowsum == 0).sum(), 6)))
    with pytest.raises(KeyError):
        np_neighbour_mean(g, "field", "paper", x)


def test_documented_errors():
    n_nodes, edges = raw_relations(50, seed=3)
    et, nt = times_for(edges, n_nodes, 3)
    build = DeviceHeteroGraph.from_edge_lists
    key = ("author", "writes", "paper")
    with pytest.raises(ValueError, match="both edge_time and a node_time"):
        build(TYPES, n_nodes, edges, {key: et[key]}, {"paper": nt["paper"]})
    for bad_id, row in ((n_nodes["paper"], 1), (-1, 1), (n_nodes["author"], 0), (-1, 0)):
        broken = OrderedDict((k, v.copy()) for k, v in edges.items())
        broken[key][row, 17] = bad_id
        with pytest.raises(IndexError, match="writes"):
            build(TYPES, n_nodes, broken)
    with pytest.raises(ValueError, match="self"):
        build(TYPES, n_nodes, {("paper", "self", "paper"): edges[("paper", "cites", "paper")]})
    with pytest.raises(ValueError, match="node types"):
        build(["t%d" % i for i in range(17)], {"t%d" % i: 2 for i in range(17)}, {})
    many = OrderedDict((("paper", "r%d" % i, "author"), np.zeros((2, 1), np.int64)) for i in range(25))
    with pytest.raises(ValueError, match="48 meta triples"):
        build(TYPES, n_nodes, many)                                       # 25 relations and their reverses
    assert len(build(TYPES, n_nodes, many, reverse=None).triples) == 25
    with pytest.raises(ValueError, match="second time"):
        build(TYPES, n_nodes, OrderedDict([(("paper", "x", "author"), np.zeros((2, 1), np.int64)),
                                           (("author", "rev_x", "paper"), np.zeros((2, 1), np.int64))]))
    with pytest.raises(ValueError, match=r"\[2, E\]"):
        build(TYPES, n_nodes, {key: np.zeros((3, 4), np.int64)})
    with pytest.raises(ValueError, match="int32 or int64"):
        build(TYPES, n_nodes, {key: np.zeros((2, 4), np.float32)})
    with pytest.raises(ValueError, match="not node types"):
        build(TYPES, n_nodes, {("paper", "in", "journal"): np.zeros((2, 1), np.int64)})
    with pytest.raises(ValueError, match="time table"):
        build(TYPES, n_nodes, edges, {key: et[key][:-1]})
    with pytest.raises(ValueError, match="time table"):
        build(TYPES, n_nodes, edges, None, {"paper": nt["paper"][:-1]})
    huge = np.broadcast_to(np.zeros((2, 1), np.int32), (2, 2 ** 31 - 1))    # no memory behind it: the size alone is refused
    with pytest.raises(RuntimeError, match=r"beyond 32-bit plan indices \(code -4\)"):
        build(TYPES, n_nodes, {key: huge})


def test_host_graph_keeps_its_old_surface():
    n_nodes, edges = raw_relations(60, seed=2)
    g = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, edges, features=features(n_nodes))
    assert g.device is None and g.csr is g.csr and g.get_types() == TYPES and g.get_meta_graph() == g.meta
    again = DeviceHeteroGraph.from_csr(TYPES, g.get_meta_graph(), n_nodes, [g.csr[g.triples.index(m)] for m in g.meta], features(n_nodes))
    assert_same_graph(again, g)
