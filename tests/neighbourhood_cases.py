"""Graphs for the neighbourhood tests (tests/test_neighbourhood.py on the CPU, tests/test_neighbourhood_gpu.py on the device) and the
oracle they are checked against: the COMPOSITION of the two existing definitions -- the whole-graph view, trimmed to the seeds.
`np_neighbourhood` is a frontier walk that never forms the whole graph; the composition forms all of it and knows nothing of
frontiers, so the two statements test each other."""
import itertools

import numpy as np

from pyhgt_amd import np_trim_graph, np_trim_to_seeds, np_whole_graph
from pyhgt_amd.neighbourhood import NeighbourhoodArrays
from pyhgt_amd.sampled import MAG_META
from pyhgt_amd.sampler import DeviceHeteroGraph
from pyhgt_amd.synth import synthetic_hetero_csr

import whole_graph_cases as W

MAG_TYPES = ["paper", "author", "field_of_study", "institution"]
FIELDS = ("order", "node_type", "edge_index", "edge_type", "edge_time", "node_feature", "out_rows")


def composition(dg, seeds, n_layers, node_time=None, max_time=None, leave_out=None, self_loops=True):
    """np_whole_graph -> np_trim_to_seeds -> np_trim_graph, as the module docstring of pyhgt_amd/neighbourhood.py states it; -> NeighbourhoodArrays"""
    a = np_whole_graph(dg, node_time, max_time, leave_out, self_loops)
    off = np.concatenate([[0], np.cumsum(dg.n_nodes)]).astype(np.int64)
    seed_rows = np.concatenate([off[dg.types.index(t)] + np.asarray(ids, dtype=np.int64).reshape(-1) for t, ids in seeds.items()]
                               + [np.zeros(0, np.int64)])
    N = int(off[-1])
    t = np_trim_to_seeds(N, a.edge_index, seed_rows, n_layers)
    node_type, edge_index, edge_type, edge_time = np_trim_graph(t, a.node_type, a.edge_index, a.edge_type, a.edge_time)
    feat = None if a.node_feature is None else a.node_feature[t.order]
    return NeighbourhoodArrays(t.order, node_type, edge_index, edge_type, edge_time, feat, t.new_id[seed_rows], t.n_rows, t.n_edges,
                               t.order - off[node_type])


def assert_same(got, want, what=""):
    """two NeighbourhoodArrays (numpy): every array equal, with the same dtype and shape"""
    assert tuple(got.n_rows) == tuple(want.n_rows) and tuple(got.n_edges) == tuple(want.n_edges), (what, got.n_rows, want.n_rows,
                                                                                                    got.n_edges, want.n_edges)
    for name in FIELDS + ("row_id",):
        g, w = getattr(got, name), getattr(want, name)
        assert (g is None) == (w is None), (what, name)
        if w is not None:
            g, w = np.asarray(g), np.asarray(w)
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name, g.dtype, w.dtype, g.shape, w.shape)


def graph_arrays(nb):
    """a NeighbourhoodGraph (device or host tensors) as NeighbourhoodArrays of numpy"""
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    return NeighbourhoodArrays(host(nb.order), host(nb.node_type), host(nb.edge_index), host(nb.edge_type), host(nb.edge_time),
                               host(nb.node_feature), host(nb.out_rows), nb.n_rows, nb.n_edges, host(nb.row_id))


# --------------------------------------------------------------------------------------------------------------- the hand graph
HAND_SEEDS = {"a1": {"a": [1]}, "a1_a1_b2": {"a": [1, 1], "b": [2]}, "d0": {"d": [0]}, "a5": {"a": [5]}}


def hand_combinations():
    """(node_time, max_time, leave_out kind, self_loops, L, seeds name): the full product the CPU test walks"""
    return list(itertools.product([False, True], [None, W.HAND_MAX_TIME], [None, "targets", "sources", "both"], [True, False], [1, 2, 3],
                                  sorted(HAND_SEEDS)))


def hand_kwargs(with_time, max_time, kind, self_loops):
    return dict(node_time=W.HAND_TIME if with_time else None, max_time=max_time, leave_out=None if kind is None else W.hand_flags(kind),
                self_loops=self_loops)


# --------------------------------------------------------------------------------------------------------------- the MAG-schema graph
def schema_graph(device=None, mean_degree=1.0, n_paper=3000, in_dim=33, seed=3):
    """test_whole_graph_gpu._schema_graph restated for the MAG schema: -> (graph on `device` or the host, node_time).  At
    mean_degree = 1.0: 7 680 nodes, 34 610 view edges."""
    n_nodes = {t: max(4, int(n_paper * f)) for t, f in zip(MAG_TYPES, [1.0, 1.5, 0.05, 0.01])}
    csr = synthetic_hetero_csr(MAG_TYPES, MAG_META, n_nodes, mean_degree=mean_degree, seed=seed, years=(2000, 2020), none_time=("AI_in",))
    rng = np.random.default_rng(seed + 1)
    feats = {t: rng.standard_normal((n_nodes[t], in_dim)).astype(np.float32) for t in MAG_TYPES}
    node_time = {t: rng.integers(2000, 2020, size=n_nodes[t]) for t in MAG_TYPES}
    return DeviceHeteroGraph.from_csr(MAG_TYPES, MAG_META, n_nodes, csr, feats, device=device), node_time


def paper_seeds(S):
    return {"paper": np.random.default_rng(S).integers(0, 3000, S)}


# --------------------------------------------------------------------------------------------------------------- cases the walk can get wrong
def _graph(types, n, nested, device=None):
    return W.make_graph(types, n, list(nested), nested, device)


def walk_cases(device=None):
    """name -> (graph, seeds, L, kwargs, check) -- check(arrays) is True iff the arrays show what the case is about (counts worked out
    by hand, in the comments)"""
    from pyhgt_amd import _lib
    out = {}
    # u0 <- u1 <- u2 and u0 <- u2: u2 is reachable at hop 1 and again at hop 2, and keeps hop 1
    g = _graph(["u"], {"u": 4}, {("u", "u", "r"): {0: [(1, None), (2, None)], 1: [(2, None), (3, None)]}}, device)
    out["hop_1_and_hop_2"] = (g, {"u": [0]}, 2, {}, lambda a: (a.n_rows == (4, 3, 1) and list(a.order) == [0, 1, 2, 3]))
    # seed u1 is seed u0's neighbour: it stays at hop 0
    out["seed_is_a_neighbour"] = (g, {"u": [0, 1]}, 1, {}, lambda a: (a.n_rows == (4, 2) and list(a.order[:2]) == [0, 1]))
    # two seeds with identical neighbour sets: every candidate of one is a duplicate
    g2 = _graph(["u", "v"], {"u": 3, "v": 5}, {("u", "v", "r"): {0: [(4, None), (1, None), (3, None)], 2: [(3, None), (4, None), (1, None)]},
                                             ("v", "u", "q"): {1: [(1, None)]}}, device)
    out["identical_neighbour_sets"] = (g2, {"u": [2, 0]}, 2, {}, lambda a: (a.n_rows == (6, 5, 2)))
    # a level that discovers nothing new: the later n_rows repeat and nothing is expanded
    g3 = _graph(["u"], {"u": 5}, {("u", "u", "r"): {0: [(1, None)], 1: [(0, None)], 3: [(4, None)]}}, device)
    out["nothing_new"] = (g3, {"u": [0]}, 4, {}, lambda a: (a.n_rows == (2, 2, 2, 2, 1)))
    # a row all of whose entries the filter drops
    g4 = _graph(["u", "v"], {"u": 3, "v": 4}, {("u", "v", "r"): {0: [(0, 2005), (1, 2006)], 1: [(2, 2000), (3, 2009)]},
                                             ("v", "u", "q"): {2: [(2, 1999)]}}, device)
    tm = {"u": np.array([2001, 2002, 2003]), "v": np.array([2000, 2001, 2002, 2003])}
    out["row_all_filtered"] = (g4, {"u": [0, 1]}, 2, dict(node_time=tm, max_time=2001),
                               lambda a: (a.n_rows == (4, 3, 2) and a.n_edges == (5, 5, 3)))
    # a type with no nodes, between two that have some
    g5 = _graph(["u", "e", "v"], {"u": 2, "e": 0, "v": 3}, {("u", "v", "r"): {1: [(2, None), (0, None)]}, ("e", "u", "s"): {},
                                                           ("v", "e", "t"): {}}, device)
    out["empty_type"] = (g5, {"u": [1], "v": [1]}, 2, {}, lambda a: (a.n_rows == (4, 4, 2)))
    out["empty_seeds"] = (g2, {}, 2, {}, lambda a: (a.n_rows == (0, 0, 0) and a.node_feature.shape == (0, 3)))
    out["empty_seed_list"] = (g2, {"v": []}, 1, {}, lambda a: (a.n_rows == (0, 0) and a.out_rows.shape == (0,)))
    # a chain as long as the deepest stack the trim takes
    Lmax = _lib.HGT_TRIM_MAX_LAYERS
    chain = _graph(["u"], {"u": Lmax + 3}, {("u", "u", "r"): {i: [(i + 1, None)] for i in range(Lmax + 2)}}, device)
    out["max_layers"] = (chain, {"u": [0]}, Lmax, {}, lambda a: (a.n_rows == tuple(range(Lmax + 1, 0, -1))))
    return out
