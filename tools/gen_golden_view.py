"""Fixture of the whole-graph view: tests/golden/view/whole_small.npz.

    python tools/gen_golden_view.py          (needs the reference tree: oracle.reference_loader.load_reference_data())

The reference has no call that turns a whole `Graph` into tensors, but its sampler does it when EVERY node is a seed: with
sampled_depth = 0 nothing is drawn, layer_data holds every node of every type -- in id order, so a node's serial is its id -- each with
the time the caller gave it, and the induction step (pyHGT/data.py:191-209) then yields every edge of the graph.  to_torch
(data.py:212-256) makes the 7-tuple of it.  This script runs exactly that on the small graph of tools/gen_golden_sampler.py and stores
what the reference returned: the node arrays, the edges as sorted rows (source, target, edge_type, edge_time) -- the reference orders
them by its dicts, the view relation-major, so tests compare multisets -- and the two dictionaries as name / value arrays.
tests/test_whole_graph.py imports the helpers below (`node_times` needs no reference; the live comparison does).
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "view", "whole_small.npz")


def _sampler_tool():
    spec = importlib.util.spec_from_file_location("gen_golden_sampler", os.path.join(ROOT, "tools", "gen_golden_sampler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _sampler_tool()


def node_times():
    """{type: int64 [n_type]}: a paper's year, an author's own year, a venue's year (the one its papers share)"""
    return {"paper": np.array([G.paper_year(p) for p in range(G.N_NODES["paper"])], dtype=np.int64),
            "author": np.array([G.author_year(a) for a in range(G.N_NODES["author"])], dtype=np.int64),
            "venue": 2000 + np.arange(G.N_NODES["venue"], dtype=np.int64),
            "empty": np.zeros(0, np.int64)}


def edge_rows(edge_index, edge_type, edge_time):
    """the edges as lexicographically sorted rows (source, target, edge_type, edge_time)"""
    rows = np.stack([np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64),
                     np.asarray(edge_type, dtype=np.int64), np.asarray(edge_time, dtype=np.int64)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def run_reference(data, graph):
    """the reference's sample_subgraph with every node a seed and sampled_depth = 0, then to_torch -> (node_feature, node_type,
    edge rows, node_dict, edge_dict)"""
    times = node_times()
    inp = {t: [[i, int(times[t][i])] for i in range(G.N_NODES[t])] for t in G.TYPES}
    feature, tm, edge_list, indxs, _ = data.sample_subgraph(graph, {10 ** 6: True}, 0, G.SAMPLED_NUMBER, inp=inp, feature_extractor=G._extractor)
    for t in G.TYPES:
        assert np.array_equal(indxs[t], np.arange(G.N_NODES[t]))          # serial = id
    nf, nt, etime, ei, et, node_dict, edge_dict = data.to_torch(feature, tm, edge_list, graph)
    return nf.numpy(), nt.numpy(), edge_rows(ei.numpy(), et.numpy(), etime.numpy()), node_dict, edge_dict


def main():
    from oracle.reference_loader import load_reference_data
    data = load_reference_data()
    edges = G.synthetic_edges()
    nf, nt, rows, node_dict, edge_dict = run_reference(data, G.reference_graph(data, edges))
    blob = {"node_feature": nf, "node_type": nt, "edges": rows,
            "node_dict/names": np.array(list(node_dict)), "node_dict/values": np.array([node_dict[k] for k in node_dict], dtype=np.int64),
            "edge_dict/names": np.array(list(edge_dict)), "edge_dict/values": np.array([edge_dict[k] for k in edge_dict], dtype=np.int64)}
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **blob)
    print("nodes", nt.size, "edges", len(rows), GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
