"""Graphs for the whole-graph view tests (tests/test_whole_graph.py on the CPU, tests/test_whole_graph_gpu.py on the device) and the
brute-force statement of the rule they are checked against: a plain loop over nested dicts, written without looking at the CSRs.

A graph here is `(types, n_nodes, meta, nested)`, nested = {(target type, source type, relation): {target id: [(source id, time or
None), ...]}} with a row's neighbours in stored order."""
import numpy as np

from pyhgt_amd.sampler import DeviceHeteroGraph, TIME_NONE

# --------------------------------------------------------------------------------------------------------------- the hand-made graph
# * ("a", "b", "link") and ("b", "a", "link") share one relation name with different target types: one relation id, two triples,
#   ordered by target type.  The dictionary rule of data.py:237-238 (a name's id is the position of its LAST triple, `self` = the number
#   of names) then leaves id 0 without a triple and gives `self` the id of the last name, "y": the arrays are still well defined --
#   they are what these tests compare -- but such a schema is no input for a plan.
# * "c" has no nodes; ("d", "b", "z") has no entry; ("c", "a", "w") has no row.
# * rows without entries at the start (a0 of link), in the middle (a2, b1, b3, d1) and at the end (a5).
# * None times (TIME_NONE in the CSR) with every kind of target time around max_time = 2001.
HAND_TYPES = ["a", "b", "c", "d"]
HAND_N = {"a": 6, "b": 5, "c": 0, "d": 3}
HAND_META = [("a", "b", "link"), ("b", "a", "link"), ("a", "a", "x"), ("d", "b", "z"), ("c", "a", "w"), ("d", "a", "y")]
HAND_NESTED = {
    ("a", "b", "link"): {1: [(0, 2001), (3, None)], 3: [(4, 2003), (1, 2000), (0, None)], 4: [(2, 2002)]},
    ("b", "a", "link"): {0: [(1, 2002)], 2: [(3, None), (4, 2001)], 4: [(0, 2004)]},
    ("a", "a", "x"): {0: [(1, 2000), (2, 2003)], 3: [(5, None)], 5: [(0, 2001)]},
    ("d", "b", "z"): {},
    ("c", "a", "w"): {},
    ("d", "a", "y"): {0: [(2, 2002)], 2: [(5, 2000), (4, None)]},
}
HAND_TIME = {"a": np.array([2000, 2001, 2002, 2003, 2004, 2000]), "b": np.array([2001, 2000, 2002, 2003, 2004]),
             "d": np.array([2002, 2001, 2000])}
HAND_MAX_TIME = 2001


def nested_to_csr(n_nodes, meta, nested):
    csr = []
    for tri in meta:
        rows = nested[tri]
        deg = np.zeros(n_nodes[tri[0]] + 1, np.int64)
        for r, nb in rows.items():
            deg[r + 1] = len(nb)
        src = [s for r in sorted(rows) for s, _ in rows[r]]
        tm = [TIME_NONE if t is None else t for r in sorted(rows) for _, t in rows[r]]
        csr.append((np.cumsum(deg).astype(np.int32), np.asarray(src, dtype=np.int32), np.asarray(tm, dtype=np.int32)))
    return csr


def make_graph(types, n_nodes, meta, nested, device=None, width=3):
    """-> DeviceHeteroGraph with features [n, width] whose first column is type index * 1000 + id"""
    feats = {}
    for i, t in enumerate(types):
        f = np.zeros((n_nodes[t], width), np.float32)
        f[:, 0] = 1000 * i + np.arange(n_nodes[t])
        f[:, 1:] = np.arange(n_nodes[t])[:, None] * 0.5
        feats[t] = f
    return DeviceHeteroGraph.from_csr(types, meta, n_nodes, nested_to_csr(n_nodes, meta, nested), feats, device=device)


def hand_graph(device=None):
    return make_graph(HAND_TYPES, HAND_N, HAND_META, HAND_NESTED, device)


def brute_force(dg, nested, node_time=None, max_time=None, leave_out=None, self_loops=True):
    """the rule of pyhgt_amd/view.py edge by edge -> (list of (source row, target row, edge_type, edge_time or None), rel_ptr)"""
    off = dict(zip(dg.types, np.concatenate([[0], np.cumsum(dg.n_nodes)])[:-1]))
    edges = []
    for tt, st, rel in dg.triples:
        tflags, sflags = (leave_out or {}).get((tt, st, rel), (None, None))
        for r in sorted(nested[(tt, st, rel)]):
            for s, t in nested[(tt, st, rel)][r]:
                if max_time is not None:
                    if t is None and node_time:
                        t = int(node_time[tt][r])
                    if t is not None and t > max_time:
                        continue
                if (tflags is not None and tflags[r]) or (sflags is not None and sflags[s]):
                    continue
                dt = int(node_time[tt][r]) - int(node_time[st][s]) + 120 if node_time else None
                edges.append((int(off[st]) + s, int(off[tt]) + r, dg.edge_dict[rel], dt))
    if self_loops:
        edges += [(i, i, dg.edge_dict["self"], 120 if node_time else None) for i in range(sum(dg.n_nodes))]
    types = [e[2] for e in edges]
    rel_ptr = [sum(1 for t in types if t < r) for r in range(len(dg.edge_dict) + 1)]
    return edges, rel_ptr


def check_against(arrays, edges, rel_ptr, has_time):
    """the definition's / a view's arrays (anything with the fields of WholeGraphArrays, as numpy) against brute_force's lists"""
    ei, et, tm = np.asarray(arrays.edge_index), np.asarray(arrays.edge_type), arrays.edge_time
    assert ei.shape == (2, len(edges)) and et.shape == (len(edges),)
    assert [tuple(int(v) for v in ei[:, e]) + (int(et[e]),) for e in range(len(edges))] == [e[:3] for e in edges]
    assert (tm is not None) == has_time
    if has_time:
        assert [int(v) for v in np.asarray(tm)] == [e[3] for e in edges]
    src32, dst32, time32, rp, _ = arrays.sorted
    assert np.array_equal(src32, ei[0]) and np.array_equal(dst32, ei[1]) and [int(v) for v in rp] == rel_ptr
    assert (time32 is None) == (not has_time) and (time32 is None or np.array_equal(time32, np.asarray(tm)))
    assert src32.dtype == dst32.dtype == rp.dtype == np.int32


def hand_flags(kind):
    """leave_out tables of the hand graph: flags on targets only, on sources only, on both sides"""
    fa = np.zeros(6, bool); fa[[3, 5]] = True
    fb = np.zeros(5, np.uint8); fb[[0, 2]] = 1
    return {"targets": {("a", "b", "link"): (fa, None), ("d", "a", "y"): (np.array([0, 0, 1], np.uint8), None)},
            "sources": {("a", "b", "link"): (None, fb), ("a", "a", "x"): (None, fa)},
            "both": {("a", "b", "link"): (fa, fb), ("b", "a", "link"): (fb, fa), ("a", "a", "x"): (fa, fa)}}[kind]


# --------------------------------------------------------------------------------------------------------------- tile-shaped graphs
def tile_graph(kind, tile, device=None, seed=0):
    """Graphs chosen against the build's tile (entries per wavefront; a workgroup takes 4 tiles).  Two types u, v; triples
    ("u", "v", "r0"), ("v", "u", "r1"), ("u", "u", "r2").  -> (DeviceHeteroGraph, nested, node_time)"""
    rng = np.random.default_rng(seed)
    types, meta = ["u", "v"], [("u", "v", "r0"), ("v", "u", "r1"), ("u", "u", "r2")]
    if kind == "long_row":                       # one row across three tiles, then rows of one
        n = {"u": 40, "v": 2 * tile + 3}
        rows0 = {3: list(range(2 * tile + 3))}
        rows0.update({r: [int(rng.integers(n["v"]))] for r in range(4, 40)})
        degs = None
    elif kind in ("multiple", "multiple_plus_one"):   # all entries (self run included) = 8 tiles exactly / one more
        n = {"u": 300, "v": 200}
        total = 8 * tile + (1 if kind == "multiple_plus_one" else 0) - 500
        degs = [total // 2, total // 4, total - total // 2 - total // 4]
        rows0 = None
    elif kind == "sparse_rows":                  # long stretches of rows without an entry: the walk gives up and searches
        n = {"u": 3000, "v": 50}
        rows0 = {r: [int(v) for v in rng.integers(n["v"], size=3)] for r in (0, 1, 700, 701, 2999)}
        degs = None
    else:
        raise KeyError(kind)
    nested = {}
    for m, (tt, st, rel) in enumerate(meta):
        if m == 0 and rows0 is not None:
            rows = rows0
        else:
            count = degs[m] if degs is not None else 60
            tgt = np.sort(rng.integers(n[tt], size=count))
            rows = {}
            for r in tgt:
                rows.setdefault(int(r), []).append(int(rng.integers(n[st])))
        nested[(tt, st, rel)] = {r: [(s, None if rng.random() < 0.2 else int(rng.integers(1990, 2012))) for s in nb]
                                 for r, nb in rows.items()}
    node_time = {t: rng.integers(1990, 2012, size=n[t]) for t in types}
    return make_graph(types, n, meta, nested, device), nested, node_time
