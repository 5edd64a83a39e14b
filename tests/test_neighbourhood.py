"""The definition of the exact neighbourhood (pyhgt_amd.neighbourhood.np_neighbourhood, a frontier walk on the CSRs) against the
composition of the two older definitions (the whole-graph view, trimmed to the seeds): every array with np.array_equal and the same
dtype.  No GPU."""
import numpy as np
import pytest
import torch

import neighbourhood_cases as NC
import whole_graph_cases as W
from pyhgt_amd import NeighbourhoodGraph, TrimmedGraph, _lib, np_neighbourhood
from pyhgt_amd.sampler import DeviceHeteroGraph


def _check(dg, seeds, L, what="", **kw):
    got, want = np_neighbourhood(dg, seeds, L, **kw), NC.composition(dg, seeds, L, **kw)
    NC.assert_same(got, want, what)
    return got


# ------------------------------------------------------------------ 1. the hand graph, every combination
@pytest.mark.parametrize("with_time", [False, True], ids=["no_time", "time"])
@pytest.mark.parametrize("max_time", [None, W.HAND_MAX_TIME])
def test_hand_graph_every_combination(with_time, max_time):
    dg = W.hand_graph()
    n = 0
    for wt, mt, kind, loops, L, name in NC.hand_combinations():
        if (wt, mt) != (with_time, max_time):
            continue
        got = _check(dg, NC.HAND_SEEDS[name], L, (kind, loops, L, name), **NC.hand_kwargs(wt, mt, kind, loops))
        assert got.n_rows[L] == len({(t, i) for t, ids in NC.HAND_SEEDS[name].items() for i in ids})
        n += 1
    assert n == 4 * 2 * 3 * 4


def test_hand_graph_counts_by_hand():
    """a1, L = 2, everything kept, worked out from HAND_NESTED and not from the code: into a1 come b0 and b3 (`link`; `x` has no row
    1), so level 1 = {b0, b3}; into b0 comes a1 (held already), b3 has no row, so level 2 is empty"""
    a = np_neighbourhood(W.hand_graph(), {"a": [1]}, 2)
    assert a.n_rows == (3, 3, 1) and list(a.order) == [1, 6, 9]
    assert a.n_edges == (2 + 1 + 1 + 2, 6, 3)              # level 0: 2 entries + 1 loop; level 1: the entry a1 -> b0 + 2 loops
    assert a.edge_type.tolist() == [1, 1, 5, 1, 5, 5]      # `link` has id 1 (its last triple), `self` the id of the last name + 1


# ------------------------------------------------------------------ 2. tile-shaped graphs, the hub row's node as a seed
@pytest.mark.parametrize("kind", ["long_row", "sparse_rows", "multiple_plus_one"])
def test_tile_graphs(kind):
    dg, nested, node_time = W.tile_graph(kind, 512)
    hub = {"long_row": 3, "sparse_rows": 700, "multiple_plus_one": int(np.argmax(np.diff(dg.csr[0][0])))}[kind]
    for kw in ({}, dict(node_time=node_time), dict(node_time=node_time, max_time=2001), dict(max_time=2001, self_loops=False)):
        got = _check(dg, {"u": [hub]}, 2, (kind, sorted(kw)), **kw)
    if kind == "long_row":
        got = np_neighbourhood(dg, {"u": [hub]}, 2)
        assert got.n_rows == (1061, 1028, 1) and got.n_edges[1:] == (2115, 1028)


# ------------------------------------------------------------------ 3. the MAG-schema graph: a walk, not a copy
@pytest.fixture(scope="module")
def mag():
    dg, node_time = NC.schema_graph()
    assert sum(dg.n_nodes) == 7680
    return dg, node_time


@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("S", [1, 8, 64])
def test_mag_schema_graph(mag, S, L):
    dg, node_time = mag
    got = _check(dg, NC.paper_seeds(S), L, (S, L), node_time=node_time)
    if L <= 2:
        assert got.n_rows[0] < 7680
    if S == 8 and L > 1:
        assert got.n_rows[0] == {2: 385, 4: 5363}[L]
    if (S, L) == (8, 2):
        _check(dg, NC.paper_seeds(S), L, "filtered", node_time=node_time, max_time=2012)


def test_mag_schema_graph_size():
    from pyhgt_amd import np_whole_graph
    dg, _ = NC.schema_graph()
    assert np_whole_graph(dg).edge_type.size == 34610


# ------------------------------------------------------------------ 4. cases the walk can get wrong
@pytest.mark.parametrize("name", sorted(NC.walk_cases()))
def test_walk_cases(name):
    dg, seeds, L, kw, check = NC.walk_cases()[name]
    got = _check(dg, seeds, L, name, **kw)
    assert check(got), (name, got.n_rows, got.n_edges)


# ------------------------------------------------------------------ 5. errors
def test_errors():
    dg = W.hand_graph()
    with pytest.raises(KeyError):
        np_neighbourhood(dg, {"nope": [0]}, 2)
    with pytest.raises(KeyError):
        np_neighbourhood(dg, {"a": [0]}, 2, leave_out={("a", "b", "nope"): (None, None)})
    for bad in ({"a": [6]}, {"a": [-1]}, {"a": [1], "c": [0]}):
        with pytest.raises(IndexError):
            np_neighbourhood(dg, bad, 2)
    for L in (0, _lib.HGT_TRIM_MAX_LAYERS + 1, 1.5):
        with pytest.raises(ValueError):
            np_neighbourhood(dg, {"a": [1]}, L)
    with pytest.raises(ValueError):                          # node_time covers every type that has nodes, or none
        np_neighbourhood(dg, {"a": [1]}, 2, node_time={"a": W.HAND_TIME["a"]})
    with pytest.raises(ValueError):
        np_neighbourhood(dg, {"a": [1]}, 2, node_time=dict(W.HAND_TIME, a=W.HAND_TIME["a"][:3]))
    far = dict(W.HAND_TIME, b=W.HAND_TIME["b"] + 500)        # a1 - b0 + 120 < 0: inside the neighbourhood of a1
    with pytest.raises(IndexError):
        np_neighbourhood(dg, {"a": [1]}, 1, node_time=far)
    with pytest.raises(IndexError):
        dg.neighbourhood({"a": [1]}, 1, node_time=far)
    np_neighbourhood(dg, {"a": [5]}, 1, node_time=far)       # a5's only in-edge comes from a0: no bad difference in ITS neighbourhood
    feats = {t: np.zeros((W.HAND_N[t], 3 if t != "b" else 4), np.float32) for t in W.HAND_TYPES}
    odd = DeviceHeteroGraph.from_csr(W.HAND_TYPES, W.HAND_META, W.HAND_N, W.nested_to_csr(W.HAND_N, W.HAND_META, W.HAND_NESTED), feats)
    with pytest.raises(ValueError):
        np_neighbourhood(odd, {"a": [1]}, 1)
    with pytest.raises(ValueError):
        odd.neighbourhood({"a": [1]}, 1)


def test_caps_of_the_host_graph():
    dg, node_time = NC.schema_graph()
    seeds = NC.paper_seeds(8)
    a = np_neighbourhood(dg, seeds, 2)
    rows2 = a.n_rows[0]
    assert dg.neighbourhood(seeds, 2, max_rows=rows2, max_edges=a.n_edges[1]).n_rows == a.n_rows
    with pytest.raises(OverflowError, match="level 2") as e:
        dg.neighbourhood(seeds, 2, max_rows=rows2 - 1)
    assert str(rows2) in str(e.value)
    with pytest.raises(OverflowError, match="level 1"):
        dg.neighbourhood(seeds, 2, max_rows=a.n_rows[1] - 1)
    with pytest.raises(OverflowError, match="edges"):
        dg.neighbourhood(seeds, 2, max_edges=a.n_edges[1] - 1)
    assert dg.neighbourhood(seeds, 2).n_rows == a.n_rows     # the next call is correct


# ------------------------------------------------------------------ 6. the host-only graph's method
@pytest.mark.parametrize("with_time", [False, True])
def test_host_graph_neighbourhood(with_time):
    dg = W.hand_graph()
    seeds = {"b": torch.tensor([2, 0, 2]), "a": [3]}
    kw = NC.hand_kwargs(with_time, W.HAND_MAX_TIME, "sources", True)
    nb = dg.neighbourhood(seeds, 2, **kw)
    a = np_neighbourhood(dg, seeds, 2, **kw)
    NC.assert_same(NC.graph_arrays(nb), a)
    assert isinstance(nb, NeighbourhoodGraph) and isinstance(nb, TrimmedGraph) and nb.gathered and not TrimmedGraph.gathered
    assert (nb.n_layers, nb.n_seeds, nb.num_types, nb.num_relations, nb.n_nodes) == (2, 4, 4, len(dg.edge_dict), a.n_rows[0])
    assert nb.seed_rows("b") == slice(0, 3) and nb.seed_rows("a") == slice(3, 4)
    assert nb.out_rows[0] == nb.out_rows[2] and all(t.device.type == "cpu" for t in nb.inputs if t is not None)
    assert [x is y for x, y in zip(nb.inputs, (nb.node_feature, nb.node_type, nb.edge_time, nb.edge_index, nb.edge_type))] == [True] * 5
    nt, ei, et, tm = nb.layer_graph(2)
    assert nt.numel() == a.n_rows[1] and ei.size(1) == a.n_edges[2] and (tm is None) == (not with_time)
    assert torch.equal(nb.row_id, nb.order - torch.tensor([0, 6, 11, 11])[nb.node_type])
    assert not hasattr(nb, "hop") and not hasattr(nb, "new_id") and not hasattr(nb, "edge_order")
