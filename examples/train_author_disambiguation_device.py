#!/usr/bin/env python
"""The author-disambiguation task of the reference (OAG/train_author_disambiguation.py) on the device: every step draws a few names,
seeds the sampler with the papers written under them and with all the authors who carry them (seeds of two types), samples the
sub-graph with the first-author edges at the seed papers masked out, and trains GNN -> Matcher(pair=True) -> pair_rank_loss; every few
steps a batch from the validation years is scored with rank_metrics (NDCG and MRR over each paper's candidates, the true author
first).  Sampling, masking, the keys, the loss and the metrics all stay on the device: no row of scores is copied to the host.

    python examples/train_author_disambiguation_device.py [--steps 30] [--papers 20000] [--no-mask]

The datasets are not available offline, so the graph is synthetic with the OAG schema: the authors fall into same-name groups of 4 to 7,
every paper has one first author (AP_write_first, at the paper's year), and a paper's features are its first author's plus noise.
--no-mask leaves the first-author edges in the batch: the model then reads the answer off an in-edge of the paper it scores."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pyhgt_amd import (GNN, Matcher, DeviceHeteroGraph, Segments, candidate_pairs, pair_rank_loss, rank_metrics,  # noqa: E402
                       sample_subgraph_device, seed_edge_mask)
from pyhgt_amd.synth import synthetic_hetero_csr  # noqa: E402
from train_device_sampler import SCHEMAS  # noqa: E402

LABEL = ("paper", "author", "AP_write_first")
TRAIN_YEARS, VALID_YEARS = (2000, 2014), (2015, 2016)


def task_graph(n_paper, feat_dim, device, seed=0, mean_degree=3.0):
    """an OAG-schema random graph with same-name author groups -> (graph, groups, first author of every paper, its year);
    groups[name] = the author ids that share the name (4 to 7 of them)"""
    types, meta, frac, none_time = SCHEMAS["oag"]
    n_nodes = {t: max(8, int(n_paper * f)) for t, f in zip(types, frac)}
    n_nodes["author"] = max(8, n_paper // 4)
    csr = synthetic_hetero_csr(types, meta, n_nodes, mean_degree=mean_degree, seed=seed, none_time=none_time)
    rng = np.random.default_rng(seed + 1)
    P, A = n_nodes["paper"], n_nodes["author"]
    cuts, at = [0], 0
    while A - at >= 8:
        at += int(rng.integers(4, 8))
        cuts.append(at)
    cuts[-1] = A                                                               # the last group takes the rest: 4 to 11 authors
    groups = [np.arange(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    first = rng.integers(0, A, size=P)
    year = rng.integers(2000, 2017, size=P)
    feats = {t: rng.standard_normal((n_nodes[t], feat_dim)).astype(np.float32) for t in types}
    feats["paper"] = feats["author"][first] + 0.5 * feats["paper"]
    order = np.argsort(first, kind="stable")
    csr[meta.index(LABEL)] = (np.arange(P + 1), first, year)
    csr[meta.index(("author", "paper", "rev_" + LABEL[2]))] = (np.concatenate([[0], np.cumsum(np.bincount(first, minlength=A))]), order,
                                                               year[order])
    return DeviceHeteroGraph.from_csr(types, meta, n_nodes, csr, feats, device=device), groups, first, year


def name_pairs(groups, first, year, years):
    """per name the papers of a time range: [(paper id, position of its author in the group, year)] (train_pairs of the script)"""
    group_of = np.empty(max(g[-1] for g in groups) + 1, np.int64)
    for n, g in enumerate(groups):
        group_of[g] = n
    pairs = {}
    for p in np.flatnonzero((year >= years[0]) & (year <= years[1])):
        n = int(group_of[first[p]])
        pairs.setdefault(n, []).append((int(p), int(first[p] - groups[n][0]), int(year[p])))
    return pairs


def draw(rng, groups, pairs, years, batch_size):
    """author_disambiguation_sample steps (1)-(2): batch_size // 4 names -> (seeds of two types, name_label); at most batch_size papers"""
    names = rng.choice(sorted(pairs), size=min(batch_size // 4, len(pairs)), replace=False)
    serial, authors, papers, name_label = {}, [], [], []
    for n in names:
        for a in groups[n]:
            serial[int(a)] = len(serial)
            authors.append([int(a), years[1]])
        for p, pos, y in pairs[n]:
            if len(papers) < batch_size:
                papers.append([p, y])
                true = int(groups[n][pos])
                name_label.append([serial[true]] + [serial[int(a)] for a in groups[n] if a != true])
    return {"paper": np.array(papers), "author": np.array(authors)}, name_label


def run(steps=30, n_paper=20000, n_hid=128, n_heads=8, n_layers=2, batch_size=128, depth=3, width=64, lr=2e-3, seed=0, device="cuda:0",
        verbose=True, masked=True, feat_dim=128, valid_every=10):
    torch.manual_seed(seed)
    dgraph, groups, first, year = task_graph(n_paper, feat_dim, device, seed)
    pairs = {"train": name_pairs(groups, first, year, TRAIN_YEARS), "valid": name_pairs(groups, first, year, VALID_YEARS)}
    window = {"train": TRAIN_YEARS, "valid": VALID_YEARS}
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    gnn = GNN(feat_dim, n_hid, T, R, n_heads, n_layers, dropout=0.2, prev_norm=True, last_norm=True, use_RTE=True).to(device)
    matcher = Matcher(n_hid).to(device)
    opt = torch.optim.AdamW(list(gnn.parameters()) + list(matcher.parameters()), lr=lr)
    rng = np.random.default_rng(seed + 2)

    def scores(split, call_seed):
        inp, name_label = draw(rng, groups, pairs[split], window[split], batch_size)
        mask = seed_edge_mask(dgraph, [LABEL[2], "rev_" + LABEL[2]], "paper", len(inp["paper"])) if masked else None
        g = sample_subgraph_device(dgraph, window[split][1], depth, width, inp, seed=call_seed, mask=mask)
        paper_key, author_key, sizes = candidate_pairs(g, name_label)
        node_rep = gnn(g[0], g[1], g[2], g[3], g[4])
        return matcher(node_rep[author_key], node_rep[paper_key], pair=True), Segments(sizes, device), g

    losses, valid, all_sizes, t0 = [], [], [], time.perf_counter()
    for step in range(steps):
        gnn.train(), matcher.train()
        res, seg, g = scores("train", seed * 100003 + 2 * step)
        loss = pair_rank_loss(res, seg)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(gnn.parameters(), 0.5)
        opt.step()
        losses.append(loss.item() / seg.n)
        all_sizes.append(seg.sizes)
        if step % valid_every == 0 or step == steps - 1:
            gnn.eval(), matcher.eval()
            with torch.no_grad():
                res, seg, g = scores("valid", seed * 100003 + 2 * step + 1)
                ndcg, rr = rank_metrics(res, sizes=seg)                         # the true author is the first of every segment
                valid.append((ndcg.mean().item(), rr.mean().item()))
            all_sizes.append(seg.sizes)
            if verbose:
                print("step %3d  loss per paper %.4f  validation NDCG %.4f  MRR %.4f  (%d papers, %d pairs, %d nodes, %d edges, "
                      "%d first-author edges in the batch)" % (step, losses[-1], valid[-1][0], valid[-1][1], seg.n, seg.total, g[1].numel(),
                                                               g[4].numel(), int((g[4] == dgraph.edge_dict[LABEL[2]]).sum())))
    torch.cuda.synchronize()
    if verbose:
        print("%.1f ms per training step; %d names" % ((time.perf_counter() - t0) / steps * 1e3, len(groups)))
    return losses, valid, np.concatenate(all_sizes)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--papers", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-mask", action="store_true")
    a = ap.parse_args()
    run(a.steps, a.papers, seed=a.seed, masked=not a.no_mask)
