#!/usr/bin/env python
"""The paper -> venue task of the reference (OAG/train_paper_venue.py) on the device sampler: every step draws seed papers from the
training years, samples their sub-graph with the label edges at the seeds masked out (sample_subgraph_device(mask=seed_edge_mask(...))),
reads the labels from the label relation of the full graph (LabelSpace.index) -- all of it on the device -- and trains GNN ->
Classifier -> nll_loss; every few steps a batch from the validation years is scored.

    python examples/train_task_device_sampler.py [--steps 30] [--papers 20000] [--no-mask] [--trim]

The datasets are not available offline, so the graph is synthetic with the OAG schema: a paper's journal (PV_Journal) is a fixed
random projection of its features and the edge carries the paper's year.  --no-mask leaves the label edges in the batch: the model then
reads the answer off an in-edge of the node it classifies, which is what the mask is for.  --trim: the seed-trimmed forward,
gnn(..., seeds=batch.seed_rows("paper")): every layer computes only the rows that still reach a seed paper."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pyhgt_amd import GNN, Classifier, DeviceHeteroGraph, LabelSpace, sample_subgraph_device, seed_edge_mask  # noqa: E402
from pyhgt_amd.synth import synthetic_hetero_csr  # noqa: E402
from train_device_sampler import SCHEMAS  # noqa: E402

LABEL = ("paper", "venue", "PV_Journal")
TRAIN_YEARS, VALID_YEARS = (None, 2014), (2015, 2016)


def task_graph(n_paper, feat_dim, device, seed=0, mean_degree=3.0):
    """an OAG-schema random graph in which every paper has one journal, argmax of a random projection of its features, at the paper's
    year; -> (graph, {type: nodes})"""
    types, meta, frac, none_time = SCHEMAS["oag"]
    n_nodes = {t: max(4, int(n_paper * f)) for t, f in zip(types, frac)}
    csr = synthetic_hetero_csr(types, meta, n_nodes, mean_degree=mean_degree, seed=seed, none_time=none_time)
    rng = np.random.default_rng(seed + 1)
    feats = {t: rng.standard_normal((n_nodes[t], feat_dim)).astype(np.float32) for t in types}
    P, V = n_nodes["paper"], n_nodes["venue"]
    venue = (feats["paper"] @ rng.standard_normal((feat_dim, V)).astype(np.float32)).argmax(axis=1)
    year = rng.integers(2000, 2020, size=P)
    order = np.argsort(venue, kind="stable")
    csr[meta.index(LABEL)] = (np.arange(P + 1), venue, year)
    csr[meta.index(("venue", "paper", "rev_PV_Journal"))] = (np.concatenate([[0], np.cumsum(np.bincount(venue, minlength=V))]), order, year[order])
    return DeviceHeteroGraph.from_csr(types, meta, n_nodes, csr, feats, device=device), n_nodes


def run(steps=30, n_paper=20000, n_hid=128, n_heads=8, n_layers=2, batch_size=128, depth=4, width=64, lr=2e-3, seed=0, device="cuda:0",
        verbose=True, masked=True, feat_dim=256, valid_every=10, trim=False):
    torch.manual_seed(seed)
    dgraph, n_nodes = task_graph(n_paper, feat_dim, device, seed)
    space = LabelSpace(dgraph, LABEL, np.arange(n_nodes["venue"]))             # cand_list: every venue is a class
    pairs = {"train": space.targets(*TRAIN_YEARS), "valid": space.targets(*VALID_YEARS)}      # (paper ids, years) by time range
    window = {"train": TRAIN_YEARS, "valid": VALID_YEARS}
    mask = seed_edge_mask(dgraph, [LABEL[2], "rev_" + LABEL[2]], "paper", batch_size) if masked else None
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    gnn = GNN(feat_dim, n_hid, T, R, n_heads, n_layers, dropout=0.2, prev_norm=True, last_norm=True, use_RTE=True).to(device)
    head = Classifier(n_hid, space.n_cols).to(device)
    opt = torch.optim.AdamW(list(gnn.parameters()) + list(head.parameters()), lr=lr)
    rng = np.random.default_rng(seed + 2)

    def batch(split, call_seed):
        ids, years = pairs[split]
        pick = rng.choice(ids.size, size=batch_size, replace=False)
        inp = {"paper": np.stack([ids[pick], years[pick]], axis=1)}
        g = sample_subgraph_device(dgraph, window[split][1], depth, width, inp, seed=call_seed, mask=mask)
        return g, g.seed_rows("paper"), space.index(g.indxs["paper"][:batch_size], *window[split])

    def seed_rep(g, x_ids):
        if trim:                                                                # the seed rows alone, from the rows that reach them
            return gnn(g[0], g[1], g[2], g[3], g[4], seeds=x_ids)
        return gnn(g[0], g[1], g[2], g[3], g[4])[x_ids]

    losses, accuracy, t0 = [], [], time.perf_counter()
    for step in range(steps):
        g, x_ids, y = batch("train", seed * 100003 + 2 * step)
        gnn.train(), head.train()
        loss = torch.nn.functional.nll_loss(head(seed_rep(g, x_ids)), y)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(gnn.parameters(), 0.5)
        opt.step()
        losses.append(loss.item())
        if step % valid_every == 0 or step == steps - 1:
            g, x_ids, y = batch("valid", seed * 100003 + 2 * step + 1)
            gnn.eval(), head.eval()
            with torch.no_grad():
                accuracy.append((head(seed_rep(g, x_ids)).argmax(dim=1) == y).float().mean().item())
            if verbose:
                print("step %3d  loss %.4f  validation accuracy %.3f  (%d nodes, %d edges, %d label edges in the batch)"
                      % (step, losses[-1], accuracy[-1], g[1].numel(), g[4].numel(), int((g[4] == dgraph.edge_dict[LABEL[2]]).sum())))
    torch.cuda.synchronize()
    if verbose:
        print("%.1f ms per training step; %d training and %d validation papers, %d classes"
              % ((time.perf_counter() - t0) / steps * 1e3, pairs["train"][0].size, pairs["valid"][0].size, space.n_cols))
    return losses, accuracy


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--papers", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-mask", action="store_true")
    ap.add_argument("--trim", action="store_true", help="the seed-trimmed forward: gnn(..., seeds=the seed rows)")
    a = ap.parse_args()
    run(a.steps, a.papers, seed=a.seed, masked=not a.no_mask, trim=a.trim)
