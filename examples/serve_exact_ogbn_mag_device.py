#!/usr/bin/env python
"""Serving exact predictions from a resident graph: "the exact L-layer output of these few papers, now".

A synthetic ogbn-mag-shaped graph stays on the device (`DeviceHeteroGraph`).  A request is a batch of paper ids:

  neighbourhood   dgraph.neighbourhood({"paper": ids}, n_layers, node_time=...) -- the exact n_layers-hop neighbourhood of the
                  papers, walked from the in-edge CSRs; its cost follows the neighbourhood, not the graph
  forward         gnn(*nb.inputs, trim=nb) -- every layer on the rows it still needs
  predict         Classifier.predict(rep)

Nothing is sampled, so nothing has to be voted on: the predictions are those of the whole-graph forward, which this example also
runs (on a graph small enough for that to be cheap) and prints next to them.

    python examples/serve_exact_ogbn_mag_device.py [--papers 20000] [--batch 64] [--layers 2]

The model is untrained: the point is that the two prediction lists agree.  Node times are those of
examples/eval_whole_graph_ogbn_mag_device.py (a paper's year; another node's latest stored time)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_eval_ogbn_mag_device as E  # noqa: E402
from eval_whole_graph_ogbn_mag_device import node_times  # noqa: E402
from pyhgt_amd import GNN, Classifier  # noqa: E402


def run(n_paper=20000, n_classes=349, batch=64, n_hid=128, n_heads=8, n_layers=2, seed=0, device="cuda:0", verbose=True, feat_dim=129,
        max_rows=None, max_edges=None):
    """-> dict(served, whole: the two prediction lists; rows, edges of the neighbourhood; graph_nodes; host_reads; max_gap: the
    largest difference between the two forwards' rows; precision)"""
    torch.manual_seed(seed)
    dgraph, n_nodes, year, _, _ = E.task_graph(n_paper, feat_dim, n_classes, device, seed)
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    gnn = GNN(feat_dim, n_hid, T, R, n_heads, n_layers, dropout=0.2, prev_norm=True, last_norm=True, use_RTE=True).to(device).eval()
    head = Classifier(n_hid, n_classes).to(device).eval()
    times = node_times(dgraph, year, E.YEARS[1] - 1)
    ids = torch.from_numpy(np.random.default_rng(seed + 3).integers(0, n_nodes["paper"], size=batch)).to(device)
    with torch.no_grad():
        nb = dgraph.neighbourhood({"paper": ids}, n_layers, node_time=times, max_rows=max_rows, max_edges=max_edges)
        rep = gnn(*nb.inputs, trim=nb)
        served = head.predict(rep)
        view = dgraph.whole_graph(node_time=times)                    # the yardstick: everything, then the same rows
        rep_whole = gnn(*view[:5])[view.type_rows("paper")][ids]
        whole = head.predict(rep_whole)
    served = (served[0] if isinstance(served, tuple) else served).tolist()
    whole = (whole[0] if isinstance(whole, tuple) else whole).tolist()
    gap = (rep - rep_whole).abs().max().item()
    if verbose:
        print("graph: %d nodes, %d edges; request: %d papers, %d layers" % (view[1].numel(), view[3].size(1), batch, n_layers))
        print("neighbourhood: %d rows, %d edges (%d host reads); rows per layer %s" % (nb.n_rows[0], nb.n_edges[1], nb.host_reads, nb.n_rows))
        print("paper      ", " ".join("%5d" % i for i in ids.tolist()[:16]))
        print("served     ", " ".join("%5d" % p for p in served[:16]))
        print("whole graph", " ".join("%5d" % p for p in whole[:16]))
        print("predictions agree: %s; max |difference of the representations| %.2e" % (served == whole, gap))
    return dict(served=served, whole=whole, rows=nb.n_rows, edges=nb.n_edges, graph_nodes=int(view[1].numel()), host_reads=nb.host_reads,
                max_gap=gap, precision=gnn.gcs[0].base_conv.precision)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--papers", type=int, default=20000)
    ap.add_argument("--classes", type=int, default=349)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(n_paper=a.papers, n_classes=a.classes, batch=a.batch, n_layers=a.layers, seed=a.seed)
