#!/usr/bin/env python
"""The paper -> field task of the reference (OAG/train_paper_field.py) on the device sampler: every step draws seed papers from the
training years, samples their sub-graph with the label edges at the seeds masked out, reads each seed's fields from the label relation
of the full graph as a short list of class columns (LabelSpace.columns) and trains GNN -> Classifier.loss(columns=, count=): the
KLDivLoss('batchmean') of the script on the raw logits, without the dense [n, C] label matrix and without the [n, C] log-probabilities.
Every few steps a batch from the validation years is scored with LabelSpace.distribution + rank_metrics (NDCG, as the script does).

    python examples/train_paper_field_device.py [--steps 30] [--papers 20000] [--torch-loss]

--torch-loss runs the chain this replaces on the same batches: LabelSpace.distribution -> Classifier.forward (torch.log_softmax under
autograd) -> torch.nn.KLDivLoss(reduction='batchmean').
The datasets are not available offline, so the graph is synthetic with the OAG schema: a paper has 1 to 4 fields (PF_in_L2), the
strongest entries of a fixed random projection of its features, and the edges carry the paper's year."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pyhgt_amd import GNN, Classifier, DeviceHeteroGraph, LabelSpace, rank_metrics, sample_subgraph_device, seed_edge_mask  # noqa: E402
from pyhgt_amd.synth import synthetic_hetero_csr  # noqa: E402
from train_device_sampler import SCHEMAS  # noqa: E402

LABEL = ("paper", "field", "PF_in_L2")
TRAIN_YEARS, VALID_YEARS = (None, 2014), (2015, 2016)
MAX_FIELDS = 4                                                                     # the longest label list: the width of LabelSpace.columns


def task_graph(n_paper, feat_dim, device, seed=0, mean_degree=3.0):
    """an OAG-schema random graph in which paper p has k_p = 1 .. MAX_FIELDS fields, the k_p strongest entries of a random projection
    of its features (k_p from the strongest one), at the paper's year; -> (graph, {type: nodes})"""
    types, meta, frac, none_time = SCHEMAS["oag"]
    n_nodes = {t: max(4, int(n_paper * f)) for t, f in zip(types, frac)}
    csr = synthetic_hetero_csr(types, meta, n_nodes, mean_degree=mean_degree, seed=seed, none_time=none_time)
    rng = np.random.default_rng(seed + 1)
    feats = {t: rng.standard_normal((n_nodes[t], feat_dim)).astype(np.float32) for t in types}
    P, F = n_nodes["paper"], n_nodes["field"]
    order = np.argsort(-(feats["paper"] @ rng.standard_normal((feat_dim, F)).astype(np.float32)), axis=1, kind="stable")[:, :MAX_FIELDS]
    k = 1 + order[:, 0] % MAX_FIELDS
    keep = np.arange(MAX_FIELDS)[None, :] < k[:, None]
    paper, field = np.nonzero(keep)[0], order[keep]                                # grouped by paper
    year = rng.integers(2000, 2020, size=P)
    by_field = np.argsort(field, kind="stable")
    csr[meta.index(LABEL)] = (np.concatenate([[0], np.cumsum(k)]), field, year[paper])
    csr[meta.index(("field", "paper", "rev_" + LABEL[2]))] = (np.concatenate([[0], np.cumsum(np.bincount(field, minlength=F))]),
                                                             paper[by_field], year[paper[by_field]])
    return DeviceHeteroGraph.from_csr(types, meta, n_nodes, csr, feats, device=device), n_nodes


def run(steps=30, n_paper=20000, n_hid=128, n_heads=8, n_layers=2, batch_size=128, depth=4, width=64, lr=2e-3, seed=0, device="cuda:0",
        verbose=True, torch_loss=False, feat_dim=256, valid_every=10, dropout=0.2, trace=None):
    """-> (training losses, validation NDCG); trace: a dict that receives the logits and the dense labels of step 0"""
    torch.manual_seed(seed)
    dgraph, n_nodes = task_graph(n_paper, feat_dim, device, seed)
    space = LabelSpace(dgraph, LABEL, np.arange(n_nodes["field"]))              # cand_list: every field is a class
    pairs = {"train": space.targets(*TRAIN_YEARS), "valid": space.targets(*VALID_YEARS)}      # (paper ids, years) by time range
    window = {"train": TRAIN_YEARS, "valid": VALID_YEARS}
    mask = seed_edge_mask(dgraph, [LABEL[2], "rev_" + LABEL[2]], "paper", batch_size)
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    gnn = GNN(feat_dim, n_hid, T, R, n_heads, n_layers, dropout=dropout, prev_norm=True, last_norm=True, use_RTE=True).to(device)
    head = Classifier(n_hid, space.n_cols).to(device)
    opt = torch.optim.AdamW(list(gnn.parameters()) + list(head.parameters()), lr=lr)
    rng = np.random.default_rng(seed + 2)
    kl = torch.nn.KLDivLoss(reduction="batchmean")

    def batch(split, call_seed):
        ids, years = pairs[split]
        pick = rng.choice(ids.size, size=batch_size, replace=False)
        inp = {"paper": np.stack([ids[pick], years[pick]], axis=1)}
        g = sample_subgraph_device(dgraph, window[split][1], depth, width, inp, seed=call_seed, mask=mask)
        return g, g.seed_rows("paper"), g.indxs["paper"][:batch_size]

    losses, ndcg, t0 = [], [], time.perf_counter()
    for step in range(steps):
        g, x_ids, papers = batch("train", seed * 100003 + 2 * step)
        gnn.train(), head.train()
        rep = gnn(g[0], g[1], g[2], g[3], g[4])[x_ids]
        if torch_loss:
            loss = kl(head(rep), space.distribution(papers, *TRAIN_YEARS))
        else:
            columns, count = space.columns(papers, *TRAIN_YEARS, width=MAX_FIELDS)
            loss = head.loss(rep, columns=columns, count=count)
        if trace is not None and step == 0:
            with torch.no_grad():
                trace["logits"] = torch.nn.functional.linear(rep, head.linear.weight, head.linear.bias).cpu()
            trace["labels"] = space.distribution(papers, *TRAIN_YEARS).cpu()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(gnn.parameters(), 0.5)
        opt.step()
        losses.append(loss.item())
        if step % valid_every == 0 or step == steps - 1:
            g, x_ids, papers = batch("valid", seed * 100003 + 2 * step + 1)
            gnn.eval(), head.eval()
            with torch.no_grad():
                scores = head(gnn(g[0], g[1], g[2], g[3], g[4])[x_ids])
            ndcg.append(rank_metrics(scores, labels=space.distribution(papers, *VALID_YEARS))[0].mean().item())
            if verbose:
                print("step %3d  loss %.4f  validation NDCG %.3f  (%d nodes, %d edges, %d label edges in the batch)"
                      % (step, losses[-1], ndcg[-1], g[1].numel(), g[4].numel(), int((g[4] == dgraph.edge_dict[LABEL[2]]).sum())))
    torch.cuda.synchronize()
    if verbose:
        print("%.1f ms per training step (%s); %d training and %d validation papers, %d classes"
              % ((time.perf_counter() - t0) / steps * 1e3, "torch log_softmax + KLDivLoss on dense labels" if torch_loss else "Classifier.loss on "
                 "label lists", pairs["train"][0].size, pairs["valid"][0].size, space.n_cols))
    return losses, ndcg


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--papers", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--torch-loss", action="store_true")
    a = ap.parse_args()
    run(a.steps, a.papers, seed=a.seed, torch_loss=a.torch_loss)
