"""Fixtures of the device sampler's task batches: tests/golden/sampler/task_small.npz.

    python tools/gen_golden_task.py          (needs the reference tree: oracle.reference_loader.load_reference_data())

Between sample_subgraph and to_torch every training script of the reference takes the edges of its label relation at the output
nodes out of the batch (OAG/train_paper_field.py:109-122, train_paper_venue.py:108-121, train_author_disambiguation.py:142-155).
This script runs the verbatim sample_subgraph on the graph and the CASES of tools/gen_golden_sampler.py, applies that step -- restated
below, it is four loops of the scripts -- to the `edge_list`, then runs the verbatim to_torch, and stores per case the edge rows in the
canonical form of det_small.npz (the node rows are det_small.npz's own).  The output nodes are the paper seeds (the first `batch_size`
papers of the batch); the label relation is PV / rev_PV, and for `two_types` (seeds of two types, the author-disambiguation shape)
also AP_write / rev_AP_write.  tests/test_task_batches.py imports the helpers below.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _sibling("gen_golden_sampler")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sampler", "task_small.npz")
NODE_TYPE = "paper"      # the type of the output nodes


def task_relations(case):
    return ["PV", "rev_PV"] + (["AP_write", "rev_AP_write"] if case == "two_types" else [])


def batch_size(case):
    return len(G.CASES[case][0][NODE_TYPE])


def mask_edge_list(edge_list, relations, node_type, below):
    """the masking step of the scripts, restated: in every relation of `relations` keep the pairs [target serial, source serial] whose
    end of type node_type -- target, source or both -- has a serial of at least `below`"""
    for tt in edge_list:
        for st in edge_list[tt]:
            for rel in edge_list[tt][st]:
                if rel in relations:
                    edge_list[tt][st][rel] = [i for i in edge_list[tt][st][rel]
                                              if (tt != node_type or i[0] >= below) and (st != node_type or i[1] >= below)]


def run_reference_task(data, graph, case):
    inp, max_time, depth = G.CASES[case]
    time_range = {(10 ** 6 if max_time is None else max_time): True}
    feature, times, edge_list, indxs, _ = data.sample_subgraph(graph, time_range, depth, G.SAMPLED_NUMBER, inp={k: list(v) for k, v in inp.items()},
                                                               feature_extractor=G._extractor)
    mask_edge_list(edge_list, set(task_relations(case)), NODE_TYPE, batch_size(case))
    nf, nt, etime, ei, et, node_dict, edge_dict = data.to_torch(feature, times, edge_list, graph)
    return G.canonical(G.TYPES, indxs, times, ei.numpy(), et.numpy(), etime.numpy(), node_dict)


def main():
    from oracle.reference_loader import load_reference_data
    data = load_reference_data()
    graph = G.reference_graph(data, G.synthetic_edges())
    det = np.load(G.GOLDEN)
    blob = {}
    for case in G.CASES:
        nodes, rows = run_reference_task(data, graph, case)
        for t in G.TYPES:                                    # the step touches no node: the node rows are those of det_small.npz
            assert np.array_equal(nodes[t], det["%s/nodes/%s" % (case, t)])
        blob["%s/edges" % case] = rows
        print(case, {t: len(nodes[t]) for t in G.TYPES}, "edges", len(rows), "of", len(det["%s/edges" % case]))
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **blob)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
