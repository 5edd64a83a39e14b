#!/usr/bin/env python
"""The node-property task of the reference (ogbn-mag/train_ogbn_mag.py, ogbn-mag/eval_ogbn_mag.py) on the device sampler.  Labels and
splits are node attributes: a resident `y` table, a `split` table (0 train, 1 valid, 2 test, by the paper's year as in ogbn-mag) and
y_train = where(split == 0, y, -1).

Training step: seed papers from the training split -> sample_subgraph_device -> GNN -> on ALL paper rows of the sub-graph
Classifier.loss(index=y_train[ids]) (rows of the other splits are ignored by their index of -1) and one
Classifier.predict(ids=ids, labels=y, split=split, n_splits=3), whose counts are the train / valid / test accuracies of the step
(train_ogbn_mag.py:165-191) without an argmax or a mask on the host.

Voted evaluation (eval_ogbn_mag.py:128-191) over the shuffled test papers, batch_size seeds at a time, in both modes of the script:
  variance_reduce   the same seeds vr_num times with different Philox seeds: one sample_subgraphs_device call, one stack, one forward,
                    one Classifier.vote with the pieces' paper counts -- one launch per piece adds the log-probabilities of the test
                    papers of that piece into the VoteTable
  sequential        one sub-graph per chunk, one Classifier.vote each
and the answer is table.accuracy(y[test]): the argmax of every test paper's sums against its label.

    python examples/train_eval_ogbn_mag_device.py [--steps 30] [--papers 20000] [--vr-num 8]

The datasets are not available offline, so the graph is synthetic with the MAG schema (paper, author, field_of_study, institution):
a paper's class is the argmax of a fixed random projection of its features."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pyhgt_amd import GNN, Classifier, DeviceHeteroGraph, VoteTable, sample_subgraph_device, sample_subgraphs_device  # noqa: E402
from pyhgt_amd.sampled import stack_device_graphs  # noqa: E402
from pyhgt_amd.synth import synthetic_hetero_csr  # noqa: E402
from train_device_sampler import SCHEMAS  # noqa: E402

YEARS = (2010, 2020)                                                               # ogbn-mag: train until 2017, valid 2018, test 2019
SPLIT_NAMES = ("train", "valid", "test")


def task_graph(n_paper, feat_dim, n_classes, device, seed=0, mean_degree=3.0):
    """a MAG-schema random graph -> (graph, n_nodes, year [P], y [P], split [P]) with the three node attributes as numpy arrays"""
    types, meta, frac, none_time = SCHEMAS["mag"]
    n_nodes = {t: max(4, int(n_paper * f)) for t, f in zip(types, frac)}
    csr = synthetic_hetero_csr(types, meta, n_nodes, mean_degree=mean_degree, seed=seed, years=YEARS, none_time=none_time)
    rng = np.random.default_rng(seed + 1)
    feats = {t: rng.standard_normal((n_nodes[t], feat_dim)).astype(np.float32) for t in types}
    y = np.argmax(feats["paper"] @ rng.standard_normal((feat_dim, n_classes)).astype(np.float32), axis=1).astype(np.int64)
    year = rng.integers(YEARS[0], YEARS[1], size=n_nodes["paper"])
    split = np.where(year <= YEARS[1] - 3, 0, np.where(year == YEARS[1] - 2, 1, 2)).astype(np.int32)
    return DeviceHeteroGraph.from_csr(types, meta, n_nodes, csr, feats, device=device), n_nodes, year, y, split


def run(steps=30, n_paper=20000, n_classes=349, n_hid=128, n_heads=8, n_layers=2, batch_size=128, depth=4, width=64, vr_num=8, lr=2e-3,
        seed=0, device="cuda:0", verbose=True, feat_dim=129, dropout=0.2, trace=None):
    """-> (training losses, per step the [train, valid, test] accuracies of the batch, {mode: VoteTable}).  trace: a dict that
    receives, downloaded, "steps" = per step (logits, paper ids) and "votes" = {mode: per vote call (logits, paper ids, piece sizes)}"""
    torch.manual_seed(seed)
    dgraph, n_nodes, year, y_host, split_host = task_graph(n_paper, feat_dim, n_classes, device, seed)
    y, split = torch.from_numpy(y_host).to(device), torch.from_numpy(split_host).to(device)
    y_train = torch.where(split == 0, y, -1)
    train_paper, test_paper = np.flatnonzero(split_host == 0), np.flatnonzero(split_host == 2)
    np.random.default_rng(43).shuffle(test_paper)                                  # eval_ogbn_mag.py:108-109
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    gnn = GNN(feat_dim, n_hid, T, R, n_heads, n_layers, dropout=dropout, prev_norm=True, last_norm=True, use_RTE=True).to(device)
    head = Classifier(n_hid, n_classes).to(device)
    opt = torch.optim.AdamW(list(gnn.parameters()) + list(head.parameters()), lr=lr)
    rng = np.random.default_rng(seed + 2)
    seeds_of = lambda ids: {"paper": np.stack([ids, year[ids]], axis=1)}
    if trace is not None:
        trace["steps"], trace["votes"] = [], {"variance_reduce": [], "sequential": []}

    def paper_rows(g, n):
        """the rows of the papers in the GNN's output: one contiguous range, in a stack too (type, then piece)"""
        return slice(g[5]["paper"][0], g[5]["paper"][0] + n)

    losses, accs, t0 = [], [], time.perf_counter()
    for step in range(steps):
        pick = rng.choice(train_paper, size=min(batch_size, train_paper.size), replace=False)
        g = sample_subgraph_device(dgraph, None, depth, width, seeds_of(pick), seed=seed * 100003 + step)
        ids = g.indxs["paper"]                                                     # every paper of the sub-graph, the seeds first
        gnn.train(), head.train()
        rep = gnn(g[0], g[1], g[2], g[3], g[4])[paper_rows(g, ids.numel())]
        loss = head.loss(rep, index=y_train[ids])
        counts = head.predict(rep, ids=ids, labels=y, split=split, n_splits=3)[1]
        if trace is not None:
            trace["steps"].append((head.logits(rep).cpu(), ids.cpu()))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(gnn.parameters(), 0.5)
        opt.step()
        losses.append(loss.item())
        accs.append([c / n if n else float("nan") for n, c in counts.tolist()])
        if verbose and (step % 5 == 0 or step == steps - 1):
            print("step %3d  loss %.4f  accuracy train %.3f valid %.3f test %.3f  (%d papers of %d nodes)"
                  % (step, losses[-1], *accs[-1], ids.numel(), g[1].numel()))
    torch.cuda.synchronize()
    t_train = (time.perf_counter() - t0) / max(steps, 1)

    gnn.eval(), head.eval()
    tables = {mode: VoteTable(n_nodes["paper"], n_classes, nodes=test_paper, device=device) for mode in ("variance_reduce", "sequential")}
    y_test = y[torch.from_numpy(test_paper).to(device)]
    with torch.no_grad():
        for lo in range(0, test_paper.size, batch_size):
            chunk, key = test_paper[lo:lo + batch_size], seed * 100003 + 7919 * (1 + lo)
            # variance_reduce: vr_num sub-graphs around the same seeds, one forward on their stack, one launch per piece
            pieces = sample_subgraphs_device(dgraph, None, depth, width, [seeds_of(chunk)] * vr_num, [key + b for b in range(vr_num)],
                                             plan=False)
            g = stack_device_graphs(pieces)
            ids = torch.cat([p.indxs["paper"] for p in pieces])
            sizes = [p.indxs["paper"].numel() for p in pieces]                     # host shapes: no synchronisation
            rep = gnn(g[0], g[1], g[2], g[3], g[4])[paper_rows(g, ids.numel())]
            head.vote(rep, tables["variance_reduce"], ids, piece_sizes=sizes)
            if trace is not None:
                trace["votes"]["variance_reduce"].append((head.logits(rep).cpu(), ids.cpu(), sizes))
            # sequential: one sub-graph per chunk
            g = sample_subgraph_device(dgraph, None, depth, width, seeds_of(chunk), seed=key)
            ids = g.indxs["paper"]
            rep = gnn(g[0], g[1], g[2], g[3], g[4])[paper_rows(g, ids.numel())]
            head.vote(rep, tables["sequential"], ids)
            if trace is not None:
                trace["votes"]["sequential"].append((head.logits(rep).cpu(), ids.cpu(), [ids.numel()]))
    acc = {mode: table.accuracy(y_test) for mode, table in tables.items()}
    if verbose:
        print("%.1f ms per training step; voted test accuracy over %d papers: variance_reduce (x%d) %.3f, sequential %.3f"
              % (t_train * 1e3, test_paper.size, vr_num, acc["variance_reduce"], acc["sequential"]))
    return losses, accs, tables


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--papers", type=int, default=20000)
    ap.add_argument("--classes", type=int, default=349)
    ap.add_argument("--vr-num", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.steps, a.papers, a.classes, vr_num=a.vr_num, seed=a.seed)
