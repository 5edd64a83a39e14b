#!/usr/bin/env python
"""Link prediction over ALL candidates on a resident graph: "which authors does the model link to this paper, and where does the true
one rank?"

A synthetic ogbn-mag-shaped graph stays on the device (`DeviceHeteroGraph`).  The papers that are asked about lose their paper-author
edges first (`label_edge_flags`: the label edges are what is to be predicted).  Then:

  candidates   ONE whole-graph forward gives the embedding of every author; `Matcher.topk(..., infer=True)` projects them once and
               keeps them in the Matcher's cache
  queries      per step a batch of papers; their exact embeddings come from `dgraph.neighbourhood`, label edges left out
  answers      Matcher.topk(authors, papers, k, infer=True): the k authors the model links to each paper, over every author, without
               the [authors, papers] score matrix
  metrics      Matcher.rank_of(authors, papers, held_out, infer=True): the exact rank of each paper's held-out author among all
               authors; MRR = mean 1 / (1 + rank), Hits@10 = mean rank < 10

    python examples/recommend_ogbn_mag_device.py [--papers 20000] [--batch 64] [--steps 3] [--k 10]

The model is untrained, so the metrics are those of chance (MRR ~ ln(A) / A over A authors): the point is the pipeline."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_eval_ogbn_mag_device as E  # noqa: E402
from eval_whole_graph_ogbn_mag_device import node_times  # noqa: E402
from pyhgt_amd import GNN, Matcher, label_edge_flags  # noqa: E402


def run(steps=3, n_paper=20000, batch=64, k=10, n_hid=128, n_heads=8, n_layers=2, seed=0, device="cuda:0", verbose=True, feat_dim=129):
    """-> dict(values, indices: the last step's answers; ranks: int64 tensor, one per asked paper; held_out: the authors they stand
    for; mrr, hits10; n_authors; cache_rows: rows of the Matcher's cache)"""
    torch.manual_seed(seed)
    dgraph, n_nodes, year, _, _ = E.task_graph(n_paper, feat_dim, 16, device, seed)
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    gnn = GNN(feat_dim, n_hid, T, R, n_heads, n_layers, dropout=0.2, prev_norm=True, last_norm=True, use_RTE=True).to(device).eval()
    matcher = Matcher(n_hid).to(device).eval()
    times = node_times(dgraph, year, E.YEARS[1] - 1)
    # the papers asked about: ones with an author; the held-out author of a paper is the first of its row
    indptr, src, _ = dgraph.csr[dgraph.triples.index(("paper", "author", "AP_write"))]
    with_author = np.flatnonzero(np.diff(indptr) > 0)
    asked = np.random.default_rng(seed + 3).choice(with_author, size=min(steps * batch, with_author.size), replace=False)
    held_out = src[indptr[asked]].astype(np.int64)
    hidden = label_edge_flags(dgraph, ["AP_write", "rev_AP_write"], "paper", torch.from_numpy(asked).to(device))
    ranks = []
    with torch.no_grad():
        view = dgraph.whole_graph(node_time=times, leave_out=hidden)
        authors = gnn(*view[:5])[view.type_rows("author")]                       # every candidate, one forward
        for s in range(0, asked.size, batch):
            ids = torch.from_numpy(asked[s:s + batch]).to(device)
            nb = dgraph.neighbourhood({"paper": ids}, n_layers, node_time=times, leave_out=hidden)
            papers = gnn(*nb.inputs, trim=nb)
            values, indices = matcher.topk(authors, papers, k, infer=True)       # (the first call projects the authors into the cache)
            rank = matcher.rank_of(authors, papers, torch.from_numpy(held_out[s:s + batch]).to(device), infer=True)
            ranks.append(rank)
            if verbose:
                print("step %d: %d papers; paper %d -> authors %s; its held-out author %d ranks %d of %d"
                      % (s // batch, ids.numel(), int(ids[0]), indices[0, :5].tolist(), int(held_out[s]), int(rank[0]), n_nodes["author"]))
    ranks = torch.cat(ranks)
    mrr = (1.0 / (1.0 + ranks.double())).mean().item()
    hits10 = (ranks < 10).double().mean().item()
    if verbose:
        print("%d papers against %d authors: MRR %.5f  Hits@10 %.5f" % (ranks.numel(), n_nodes["author"], mrr, hits10))
    return dict(values=values, indices=indices, ranks=ranks, held_out=torch.from_numpy(held_out).to(device), mrr=mrr, hits10=hits10,
                n_authors=n_nodes["author"], cache_rows=int(matcher.cache.size(0)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--papers", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(steps=a.steps, n_paper=a.papers, batch=a.batch, k=a.k, n_layers=a.layers, seed=a.seed)
