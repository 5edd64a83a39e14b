#!/usr/bin/env python
"""The training loop of examples/train_synthetic.py with its batches drawn by the device sampler: a synthetic MAG- or OAG-shaped
graph is put on the device once (DeviceHeteroGraph), and every step samples a fresh sub-graph around random seed papers with
sample_subgraph_device (instead of sample_subgraph + to_torch on the host) -> GNN -> Classifier -> nll_loss -> backward -> step.

    python examples/train_device_sampler.py [--schema mag|oag] [--steps 30] [--stack B] [--papers 20000] [--trim]

--stack B: B sampled batches per optimizer step, drawn by one sample_subgraphs_device call (one pass of launches, one host read) and
stacked on the device (stack_device_graphs); the pieces are sampled without a plan.  --stack 1 is the single call.
--trim: the seed-trimmed forward, gnn(..., seeds=the seed rows): every layer computes only the rows that still reach a seed, and the
result is the seed rows alone ("Seed-trimmed forward").
The datasets are not available offline, so the task is synthetic: a paper's label is a fixed random projection of its features."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import GNN, Classifier, DeviceHeteroGraph, sample_subgraph_device, sample_subgraphs_device  # noqa: E402
from pyhgt_amd._lib import HGT_SAMPLER_MAX_BATCH  # noqa: E402
from pyhgt_amd.sampled import MAG_META, OAG_META, stack_device_graphs  # noqa: E402
from pyhgt_amd.synth import synthetic_hetero_csr  # noqa: E402

SCHEMAS = {
    # types, meta triples, nodes per type as a fraction of the papers, relations whose edges carry no time
    "mag": (["paper", "author", "field_of_study", "institution"], MAG_META, [1.0, 1.5, 0.05, 0.01], ("AI_in",)),
    "oag": (["paper", "author", "field", "venue", "affiliation"], OAG_META, [1.0, 1.5, 0.05, 0.005, 0.02], ("in",)),
}


def resident_graph(schema, n_paper, feat_dim, device, seed=0, mean_degree=3.0):
    """a random graph of the schema on the device (or device=None: host only) with features and paper labels"""
    types, meta, frac, none_time = SCHEMAS[schema]
    n_nodes = {t: max(4, int(n_paper * f)) for t, f in zip(types, frac)}
    csr = synthetic_hetero_csr(types, meta, n_nodes, mean_degree=mean_degree, seed=seed, none_time=none_time)
    rng = np.random.default_rng(seed + 1)
    feats = {t: rng.standard_normal((n_nodes[t], feat_dim)).astype(np.float32) for t in types}
    return DeviceHeteroGraph.from_csr(types, meta, n_nodes, csr, feats, device=device), n_nodes


def run(schema="mag", steps=30, n_paper=20000, n_hid=128, n_heads=8, n_layers=2, n_classes=16, batch_size=128, depth=4, width=64, lr=2e-3,
        seed=0, device="cuda:0", verbose=True, stack=1, device_optimizer=False, trim=False):
    torch.manual_seed(seed)
    feat_dim = 129 if schema == "mag" else 256
    dgraph, n_nodes = resident_graph(schema, n_paper, feat_dim, device, seed)
    proj = torch.randn(feat_dim, n_classes, generator=torch.Generator().manual_seed(seed))
    labels = (dgraph.features[0] @ proj.to(device)).argmax(dim=1)          # a learnable synthetic task on the papers
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    gnn = GNN(feat_dim, n_hid, T, R, n_heads, n_layers, dropout=0.2, prev_norm=True, last_norm=True, use_RTE=True).to(device)
    head = Classifier(n_hid, n_classes).to(device)
    if device_optimizer:   # clip + AdamW in three launches of pyhgt_amd's own kernels; the head stays out of the norm, as below
        import pyhgt_amd
        opt = pyhgt_amd.AdamW([dict(params=list(gnn.parameters())), dict(params=list(head.parameters()), clip=False)], lr=lr, max_norm=0.5)
    else:
        opt = torch.optim.AdamW(list(gnn.parameters()) + list(head.parameters()), lr=lr)
    rng = np.random.default_rng(seed + 2)
    losses, t_sample, t0 = [], 0.0, time.perf_counter()
    for step in range(steps):
        ts = time.perf_counter()
        inps = []
        for b in range(stack):
            ids = rng.choice(n_nodes["paper"], size=batch_size, replace=False)
            inps.append({"paper": np.stack([ids, np.full(batch_size, 2015)], axis=1)})
        keys = [seed * 100003 + step * stack + b for b in range(stack)]
        if stack == 1:
            pieces = [sample_subgraph_device(dgraph, 2015, depth, width, inps[0], seed=keys[0])]
        else:                                                               # the same pieces as `stack` single calls, bit for bit
            pieces = []
            for lo in range(0, stack, HGT_SAMPLER_MAX_BATCH):
                hi = min(stack, lo + HGT_SAMPLER_MAX_BATCH)
                pieces += sample_subgraphs_device(dgraph, 2015, depth, width, inps[lo:hi], keys[lo:hi], plan=False)
        if stack == 1:
            g, seeds = pieces[0], slice(0, batch_size)                      # the seeds are the first papers of the batch
        else:
            g = stack_device_graphs(pieces)
            seeds = torch.cat([g.rows(b, "paper", range(batch_size)) for b in range(stack)])
        y = torch.cat([labels[p.indxs["paper"][:batch_size]] for p in pieces])
        t_sample += time.perf_counter() - ts
        gnn.train(), head.train()
        if trim:                                                            # the seed rows alone, from the rows that reach them
            rows = pieces[0].seed_rows("paper") if stack == 1 else seeds
            loss = torch.nn.functional.nll_loss(head(gnn(g[0], g[1], g[2], g[3], g[4], seeds=rows)), y)
        else:
            rep = gnn(g[0], g[1], g[2], g[3], g[4])
            loss = torch.nn.functional.nll_loss(head(rep[seeds]), y)
        opt.zero_grad()
        loss.backward()
        if not device_optimizer:
            torch.nn.utils.clip_grad_norm_(gnn.parameters(), 0.5)
        opt.step()
        losses.append(loss.item())
        if verbose and (step % 5 == 0 or step == steps - 1):
            print("step %3d  loss %.4f  (%d nodes, %d edges)" % (step, losses[-1], g[1].numel(), g[4].numel()))
    torch.cuda.synchronize()
    if verbose:
        print("%.1f ms per training step, of which %.1f ms host time in the sampler calls" % ((time.perf_counter() - t0) / steps * 1e3,
                                                                                           t_sample / steps * 1e3))
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--schema", default="mag", choices=["mag", "oag"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--papers", type=int, default=20000)
    ap.add_argument("--stack", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-optimizer", action="store_true", help="pyhgt_amd.AdamW(max_norm=0.5) in place of clip_grad_norm_ + torch.optim.AdamW")
    ap.add_argument("--trim", action="store_true", help="the seed-trimmed forward: gnn(..., seeds=the seed rows)")
    a = ap.parse_args()
    run(a.schema, a.steps, a.papers, seed=a.seed, stack=a.stack, device_optimizer=a.device_optimizer, trim=a.trim)
