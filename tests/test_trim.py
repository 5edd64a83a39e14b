"""CPU tests of the seed-trim definition pyhgt_amd.np_trim_to_seeds: against a brute force (boolean reachability by repeated dense
adjacency products), on hand-built cases, and its invariants on random graphs; the header and the binding declare the new symbols."""
import os
import re

import numpy as np
import pytest

from pyhgt_amd import _lib, np_trim_graph, np_trim_to_seeds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute(n, ei, seeds, L):
    """hop by dense products: reach_k = the nodes with a directed path of exactly <= k edges into a seed."""
    src, dst = np.asarray(ei, np.int64).reshape(2, -1)
    A = np.zeros((n, n), bool)                       # A[s, t]: an edge s -> t
    A[src, dst] = True
    reach = np.zeros(n, bool)
    reach[np.asarray(seeds, np.int64)] = True
    hop = np.where(reach, 0, -1).astype(np.int32)
    for k in range(1, L + 1):
        nxt = reach | (A.astype(np.int64) @ reach.astype(np.int64) > 0)
        hop[nxt & ~reach] = k
        reach = nxt
    rows = sorted((int(h), v) for v, h in enumerate(hop) if h >= 0)
    order = np.array([v for _, v in rows], np.int64)
    new_id = np.full(n, -1, np.int64)
    new_id[order] = np.arange(order.size)
    edges = sorted((int(hop[t]), e) for e, t in enumerate(dst) if 0 <= hop[t] <= L - 1)
    edge_order = np.array([e for _, e in edges], np.int64)
    n_rows = tuple(int(((hop >= 0) & (hop <= L - k)).sum()) for k in range(L + 1))
    ne = [sum(1 for h, _ in edges if h <= L - l) for l in range(1, L + 1)]
    return hop, order, new_id, edge_order, n_rows, tuple([ne[0]] + ne)


def _same(t, ref):
    for got, want, name in zip(t, ref, t._fields):
        if isinstance(want, tuple):
            assert got == want, name
        else:
            assert got.dtype == want.dtype and np.array_equal(got, want), name


def hand_built_cases():
    """name -> (n_nodes, edge_index, seeds, n_layers); shared with the GPU tests."""
    chain = np.array([np.arange(9), np.arange(1, 10)])               # 0 -> 1 -> ... -> 9
    return {
        "chain": (10, chain, [9], 3),
        "seed_without_in_edges": (5, np.array([[0, 0, 1], [1, 2, 2]]), [0], 2),
        "self_loops": (4, np.array([[0, 1, 1, 2, 3], [0, 1, 0, 1, 3]]), [0], 2),
        "parallel_edges": (3, np.array([[1, 2, 1, 1], [0, 1, 0, 0]]), [0], 2),
        "repeated_unsorted_seeds": (8, np.array([[0, 1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 7]]), [6, 2, 6, 2, 2], 2),
        "every_node_a_seed": (6, np.array([[0, 1, 2, 3, 4, 5, 0], [1, 2, 3, 4, 5, 0, 3]]), [3, 0, 5, 1, 4, 2], 3),
        "one_layer": (6, np.array([[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]]), [5, 3], 1),
    }


@pytest.mark.parametrize("name", sorted(hand_built_cases()))
def test_hand_built_case_equals_the_brute_force(name):
    n, ei, seeds, L = hand_built_cases()[name]
    _same(np_trim_to_seeds(n, ei, seeds, L), _brute(n, ei, seeds, L))


def test_chain_keeps_four_rows_and_three_edges_and_drops_the_edge_into_the_last_row():
    n, ei, seeds, L = hand_built_cases()["chain"]
    t = np_trim_to_seeds(n, ei, seeds, L)
    assert t.order.tolist() == [9, 8, 7, 6] and t.n_rows == (4, 3, 2, 1)
    assert t.edge_order.tolist() == [8, 7, 6] and t.n_edges == (3, 3, 2, 1)
    assert t.hop.tolist() == [-1] * 6 + [3, 2, 1, 0]
    assert 5 not in t.edge_order.tolist()            # 5 -> 6 ends in the hop = L row: layer 1 does not compute that row
    assert t.new_id.tolist() == [-1] * 6 + [3, 2, 1, 0]


def test_seed_without_in_edges_is_the_only_row():
    t = np_trim_to_seeds(*hand_built_cases()["seed_without_in_edges"])
    assert t.order.tolist() == [0] and t.n_rows == (1, 1, 1) and t.n_edges == (0, 0, 0) and t.edge_order.size == 0


def test_self_loops_are_kept_with_their_row():
    t = np_trim_to_seeds(*hand_built_cases()["self_loops"])
    assert t.hop.tolist() == [0, 1, 2, -1]
    assert t.edge_order.tolist() == [0, 2, 1, 3]     # into hop 0: the loop at 0 and 1 -> 0; into hop 1: the loop at 1 and 2 -> 1
    assert t.n_edges == (4, 4, 2)


def test_parallel_edges_both_stay_in_their_order():
    t = np_trim_to_seeds(*hand_built_cases()["parallel_edges"])
    assert t.edge_order.tolist() == [0, 2, 3, 1] and t.n_edges == (4, 4, 3)


def test_repeated_unsorted_seeds_count_once():
    n, ei, seeds, L = hand_built_cases()["repeated_unsorted_seeds"]
    t = np_trim_to_seeds(n, ei, seeds, L)
    assert t.n_rows[L] == 2 and t.order[:2].tolist() == [2, 6]
    assert t.new_id[np.array(seeds)].tolist() == [1, 0, 1, 0, 0]
    _same(t, np_trim_to_seeds(n, ei, [2, 6], L))


def test_every_node_a_seed_keeps_everything_in_place():
    n, ei, seeds, L = hand_built_cases()["every_node_a_seed"]
    t = np_trim_to_seeds(n, ei, seeds, L)
    assert t.order.tolist() == list(range(n)) and t.edge_order.tolist() == list(range(ei.shape[1]))
    assert t.n_rows == (n,) * (L + 1) and t.n_edges == (ei.shape[1],) * (L + 1)


def test_one_layer():
    t = np_trim_to_seeds(*hand_built_cases()["one_layer"])
    assert t.order.tolist() == [3, 5, 2, 4] and t.n_rows == (4, 2) and t.edge_order.tolist() == [2, 4] and t.n_edges == (2, 2)


def test_out_of_range_ids_and_layer_counts_raise():
    ei = np.array([[0, 1], [1, 2]])
    for seeds in ([3], [-1]):
        with pytest.raises(IndexError):
            np_trim_to_seeds(3, ei, seeds, 2)
    for bad in (np.array([[0, 3], [1, 2]]), np.array([[0, 1], [1, -2]])):
        with pytest.raises(IndexError):
            np_trim_to_seeds(3, bad, [0], 2)
    for L in (0, -1, _lib.HGT_TRIM_MAX_LAYERS + 1):
        with pytest.raises(ValueError):
            np_trim_to_seeds(3, ei, [0], L)
    t = np_trim_to_seeds(3, np.zeros((2, 0), np.int64), [], 2)          # everything empty is valid
    assert t.n_rows == (0, 0, 0) and t.n_edges == (0, 0, 0) and t.hop.tolist() == [-1, -1, -1]
    t = np_trim_to_seeds(0, np.zeros((2, 0), np.int64), [], 1)
    assert t.n_rows == (0, 0) and t.hop.size == 0


RANDOM = [(n, e, s, L, seed) for seed, (n, e, s) in enumerate([(30, 60, 2), (64, 200, 3), (150, 300, 5), (300, 1500, 4), (300, 400, 20)])
          for L in (1, 2, 3, 4)]


def _random_graph(n, e, s, seed):
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, n, size=(2, e))
    ei[:, : e // 10] = ei[:, e // 10: 2 * (e // 10)]                     # parallel edges
    ei[1, -3:] = ei[0, -3:]                                              # self loops
    return ei, rng.integers(0, n, size=s)


@pytest.mark.parametrize("n,e,s,L,seed", RANDOM)
def test_random_graphs_equal_the_brute_force_and_keep_the_invariants(n, e, s, L, seed):
    ei, seeds = _random_graph(n, e, s, seed)
    t = np_trim_to_seeds(n, ei, seeds, L)
    _same(t, _brute(n, ei, seeds, L))
    assert all(a >= b for a, b in zip(t.n_rows, t.n_rows[1:])) and all(a >= b for a, b in zip(t.n_edges, t.n_edges[1:]))
    assert t.n_rows[L] == np.unique(seeds).size
    ntype = np.arange(n) % 3
    etype = np.arange(e) % 5
    nt, ei_new, et, tm = np_trim_graph(t, ntype, ei, etype, etype + 100)
    assert np.array_equal(nt, ntype[t.order]) and np.array_equal(et, etype[t.edge_order]) and np.array_equal(tm, et + 100)
    assert ei_new.min(initial=0) >= 0
    for l in range(1, L + 1):
        src, dst = ei_new[:, :t.n_edges[l]]
        assert (src < t.n_rows[l - 1]).all(), "a source outside the rows layer %d reads" % l
        assert (dst < t.n_rows[l]).all(), "a target layer %d does not compute" % l
        # every target of the layer has all its in-edges of the untrimmed graph, with their multiplicity
        targets = t.order[:t.n_rows[l]]
        for v in targets[:: max(1, targets.size // 40)]:
            want = sorted(ei[0][ei[1] == v].tolist())
            got = sorted(t.order[src[dst == t.new_id[v]]].tolist())
            assert got == want, (l, v)


def test_header_and_binding_declare_the_trim_symbols_under_abi_8():
    header = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    assert re.search(r"#define HGT_ABI_VERSION 8\b", header) and _lib.ABI_VERSION == 8
    assert re.search(r"#define HGT_TRIM_MAX_LAYERS (\d+)", header).group(1) == str(_lib.HGT_TRIM_MAX_LAYERS)
    assert _lib.HGT_TRIM_MAX_LAYERS >= 8
    for name in ("hgt_trim_tmp_bytes", "hgt_trim_hops", "hgt_trim_fill"):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1, name
    makefile = open(os.path.join(ROOT, "pyhgt_amd", "csrc", "Makefile")).read()
    assert "hgt_trim.hip" in makefile
