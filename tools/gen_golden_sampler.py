"""Fixtures of the device sampler's deterministic regime: tests/golden/sampler/det_small.npz.

    python tools/gen_golden_sampler.py          (needs the reference tree: oracle.reference_loader.load_reference_data())

The reference's sample_subgraph (pyHGT/data.py:87-210) draws no random number when sampled_number exceeds every degree and every budget
size; its output is then a function of the graph and the seeds alone, and pyhgt_amd.sampler must reproduce it exactly.  This script
builds a small synthetic `Graph`, runs the verbatim sample_subgraph + to_torch on it for CASES and stores

  * the graph as plain arrays (per meta triple: target ids, source ids, times in insertion order; INT32_MIN = None), and
  * per case what the reference returned, relabelled by original id: per type the sorted (id, time) pairs, and the sorted
    rows (relation, target type, target id, source type, source id, edge time).

The graph (4 types, 5 meta triples) is built so that the reference's rules and the sampler's coincide: a source's time is a function
of the source (paper: its year; author: its own year; venue: None, inherited from papers that all share the venue's year), the seeds
touch paper, author and venue in get_types() order, papers of year 2004 are newer than max_time = 2003, `empty` has no node.
tests/test_sampler.py imports the helpers below (the graph builder needs no reference; the live comparison does).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "sampler", "det_small.npz")
NONE = -2 ** 31
TYPES = ["paper", "author", "venue", "empty"]
N_NODES = {"paper": 40, "author": 25, "venue": 5, "empty": 0}
META = [("paper", "paper", "PP_cite"), ("paper", "author", "AP_write"), ("paper", "venue", "PV"), ("author", "paper", "rev_AP_write"),
        ("venue", "paper", "rev_PV")]
SAMPLED_NUMBER = 64      # above every degree and every budget size of the graph
# name -> (seeds {type: [[id, time]]}, max_time or None, depth)
CASES = {
    "depth2": ({"paper": [[0, 2000], [1, 2001], [2, 2002], [3, 2003]]}, 2003, 2),
    "depth1": ({"paper": [[0, 2000], [1, 2001], [2, 2002], [3, 2003]]}, 2003, 1),
    "depth0": ({"paper": [[0, 2000], [1, 2001], [2, 2002], [3, 2003], [5, 2000], [6, 2001]]}, 2003, 0),
    "no_filter": ({"paper": [[0, 2000], [1, 2001], [2, 2002], [3, 2003]]}, None, 2),
    "two_types": ({"paper": [[0, 2000], [7, 2002]], "author": [[4, 2000], [9, 2001]]}, 2003, 1),
}


def paper_year(p):
    return 2000 + p % 5


def author_year(a):
    return 2000 + a % 4


def synthetic_edges(seed=5):
    """-> {triple index: (tgt int64[], src int64[], time int64[])} in insertion order (no duplicates of (tgt, src) in a triple)"""
    rng = np.random.default_rng(seed)
    P, A = N_NODES["paper"], N_NODES["author"]
    cite, write = [], []
    for p in range(P):
        for q in rng.choice(P, size=rng.integers(1, 5), replace=False):
            if q != p:
                cite.append((p, int(q)))
        for a in rng.choice(A, size=rng.integers(1, 4), replace=False):
            write.append((p, int(a)))
    arr = lambda rows: np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    cite, write = arr(cite), arr(write)
    venue = np.stack([np.arange(P), np.arange(P) % 5], axis=1)
    out = {0: (cite[:, 0], cite[:, 1], np.array([paper_year(q) for q in cite[:, 1]])),
           1: (write[:, 0], write[:, 1], np.array([author_year(a) for a in write[:, 1]])),
           2: (venue[:, 0], venue[:, 1], np.full(P, NONE)),
           3: (write[:, 1], write[:, 0], np.array([paper_year(p) for p in write[:, 0]])),
           4: (venue[:, 1], venue[:, 0], np.array([paper_year(p) for p in venue[:, 0]]))}
    return {k: tuple(np.asarray(a, dtype=np.int64) for a in v) for k, v in out.items()}


def csr_from_edges(edges):
    """the arrays of DeviceHeteroGraph.from_csr: per triple (indptr, src, time), a target's neighbours in insertion order"""
    csr = []
    for m, (tt, _, _) in enumerate(META):
        tgt, src, tm = edges[m]
        order = np.argsort(tgt, kind="stable")
        indptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=N_NODES[tt]))])
        csr.append((indptr.astype(np.int32), src[order].astype(np.int32), tm[order].astype(np.int32)))
    return csr


def reference_graph(data, edges):
    """the same graph as the reference's `Graph` (data.py:19-83), filled through its own edge_list / node_feature attributes"""
    g = data.Graph()
    for t in TYPES:
        g.node_feature[t] = list(range(N_NODES[t]))
    for m, (tt, st, rel) in enumerate(META):
        for v, s, tm in zip(*edges[m]):
            g.edge_list[tt][st][rel][int(v)][int(s)] = None if tm == NONE else int(tm)
    return g


def _extractor(layer_data, graph):
    """feature_extractor of sample_subgraph (data.py:176): the original id as the only feature"""
    feature, times, indxs = {}, {}, {}
    for t in graph.get_types():
        ids = list(layer_data[t].keys()) if t in layer_data else []
        indxs[t] = np.asarray(ids, dtype=np.int64)
        times[t] = np.asarray([layer_data[t][k][1] for k in ids], dtype=np.int64)
        feature[t] = indxs[t].astype(np.float32).reshape(-1, 1)
    return feature, times, indxs, []


def canonical(types, indxs, times, edge_index, edge_type, edge_time, node_dict):
    """relabel by original id: -> ({type: sorted [id, time] rows}, sorted rows (rel, tgt type, tgt id, src type, src id, edge time))"""
    ids = np.concatenate([np.asarray(indxs[t], dtype=np.int64) for t in types]) if types else np.zeros(0, np.int64)
    ntype = np.concatenate([np.full(len(indxs[t]), node_dict[t][1], dtype=np.int64) for t in types])
    nodes = {}
    for t in types:
        rows = np.stack([np.asarray(indxs[t], dtype=np.int64), np.asarray(times[t], dtype=np.int64)], axis=1).reshape(-1, 2)
        nodes[t] = rows[np.argsort(rows[:, 0], kind="stable")]
    src, tgt = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    rows = np.stack([np.asarray(edge_type, dtype=np.int64), ntype[tgt], ids[tgt], ntype[src], ids[src], np.asarray(edge_time, dtype=np.int64)], axis=1)
    return nodes, rows[np.lexsort(rows.T[::-1])]


def run_reference(data, graph, case):
    inp, max_time, depth = CASES[case]
    time_range = {(10 ** 6 if max_time is None else max_time): True}
    feature, times, edge_list, indxs, _ = data.sample_subgraph(graph, time_range, depth, SAMPLED_NUMBER, inp={k: list(v) for k, v in inp.items()},
                                                               feature_extractor=_extractor)
    nf, nt, etime, ei, et, node_dict, edge_dict = data.to_torch(feature, times, edge_list, graph)
    assert edge_dict == {m[2]: i for i, m in enumerate(META)} | {"self": len(META)}
    return canonical(TYPES, indxs, times, ei.numpy(), et.numpy(), etime.numpy(), node_dict)


def main():
    from oracle.reference_loader import load_reference_data
    data = load_reference_data()
    edges = synthetic_edges()
    graph = reference_graph(data, edges)
    blob = {}
    for m in range(len(META)):
        for k, a in zip(("tgt", "src", "time"), edges[m]):
            blob["edges/%d/%s" % (m, k)] = a
    for case in CASES:
        nodes, rows = run_reference(data, graph, case)
        for t in TYPES:
            blob["%s/nodes/%s" % (case, t)] = nodes[t]
        blob["%s/edges" % case] = rows
        print(case, {t: len(nodes[t]) for t in TYPES}, "edges", len(rows))
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **blob)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
