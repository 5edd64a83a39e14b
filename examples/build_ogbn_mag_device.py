#!/usr/bin/env python
"""From raw ogbn-mag-shaped arrays to a sampled batch and a forward pass without leaving the device: what the reference does in
ogbn-mag/preprocess_ogbn_mag.py (a Python step per edge, then scipy) followed by sample_subgraph + to_torch.

    python examples/build_ogbn_mag_device.py [--scale 0.05] [--dim 128]

The dataset is not available offline, so the raw arrays are synthetic (pyhgt_amd.synth.synthetic_mag_raw): four relations as
`edge_index_dict`, paper features and paper years -- the form OGB ships.  Steps:
  1  DeviceHeteroGraph.from_edge_lists: the resident CSRs of the eight meta triples (four relations and their reverses), the edges
     taking the year of their paper end (lines 29-42)
  2  the features of the types that have none (lines 69-99): authors and fields the mean of their papers' features, institutions the
     mean of their authors' COMPUTED rows, every type with log10(degree) as its last column
  3  one batch around random seed papers with sample_subgraph_device, one GNN forward on it"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import GNN, DeviceHeteroGraph, neighbour_mean, sample_subgraph_device  # noqa: E402
from pyhgt_amd.synth import synthetic_mag_raw  # noqa: E402


def build(scale=0.05, dim=128, device="cuda:0", seed=0, verbose=True):
    types, n_nodes, edges, x_paper, years = synthetic_mag_raw(scale, dim, seed)
    edges = {k: v.to(device) for k, v in edges.items()}
    x_paper, years = x_paper.to(device), years.to(device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dg = DeviceHeteroGraph.from_edge_lists(types, n_nodes, edges, node_time={"paper": years}, device=device)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    # the script's log10(degree) is -inf at degree 0; ogbn-mag has no such node, the synthetic graph does, so it is clamped here
    last = {t: torch.log10(dg.degree[t].clamp(min=1).float()) for t in types}
    feat = {t: torch.empty(n_nodes[t], dim + 1, device=device) for t in types}
    feat["paper"][:, :dim] = x_paper
    for t in ("author", "field_of_study"):
        neighbour_mean(dg, t, "paper", x_paper, out=feat[t][:, :dim])
    neighbour_mean(dg, "institution", "author", feat["author"][:, :dim], out=feat["institution"][:, :dim])      # a column slice, read in place
    for t in types:
        feat[t][:, dim] = last[t]
    dg.set_features(feat)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if verbose:
        print("graph: %s nodes, %d edges in %d meta triples; built in %.1f ms, features in %.1f ms" % (
            dict(n_nodes), sum(c[1].numel() for c in dg.csr_dev), len(dg.triples), (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    return dg, n_nodes


def run(scale=0.05, dim=128, device="cuda:0", seed=0, batch_size=64, verbose=True):
    dg, n_nodes = build(scale, dim, device, seed, verbose)
    torch.manual_seed(seed)
    ids = torch.randperm(n_nodes["paper"])[:batch_size]
    inp = {"paper": torch.stack([ids, torch.full_like(ids, 2019)], dim=1).numpy()}
    g = sample_subgraph_device(dg, 2019, 2, 32, inp, seed=seed)
    gnn = GNN(dim + 1, 64, len(dg.types), len(dg.edge_dict), 4, 2, dropout=0.2, prev_norm=True, last_norm=True, use_RTE=True).to(device).eval()
    with torch.no_grad():
        rep = gnn(g[0], g[1], g[2], g[3], g[4])
    torch.cuda.synchronize()
    if verbose:
        print("batch: %d nodes, %d edges; representation %s, finite: %s" % (g[1].numel(), g[4].numel(), tuple(rep.shape),
                                                                           bool(torch.isfinite(rep).all())))
    return dg, g, rep


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.05, help="node and edge counts as a fraction of ogbn-mag's")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.scale, a.dim, seed=a.seed)
