#!/usr/bin/env python
"""End-to-end training loop in the shape of the reference's scripts (ogbn-mag/train_ogbn_mag.py:141-198,
OAG/train_paper_field.py:218-279): sampled batch -> to_device_graph (instead of to_torch + .to(device)) -> GNN -> Classifier
-> nll_loss -> backward -> optimizer step, on sampler-shaped synthetic batches (the datasets are not available offline).

    python examples/train_synthetic.py [--schema mag|oag] [--steps 30] [--conv hgt|dense_hgt] [--n-hid 128] [--n-heads 8] [--stack B]

--stack B: B sampled batches per optimizer step, stacked on the device into one block-diagonal graph (stack_device_graphs): one
forward and one backward for the launch count of one batch.  It is ONE optimizer step over B batches (a B times larger batch),
and its dropout masks are drawn over the stacked rows: another draw than B separate steps'.

Everything on the hot path runs on the HIP kernels of pyhgt_amd (forward and backward); torch supplies the optimizer, the loss
and the autograd boundary.  --device-optimizer: the clip and the AdamW update run on pyhgt_amd's kernels as well."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import GNN, Classifier  # noqa: E402
from pyhgt_amd.sampled import stack_device_graphs, synthetic_sampled_batch, to_device_graph  # noqa: E402


def run(schema="mag", steps=30, conv="hgt", n_hid=128, n_heads=8, n_layers=2, n_classes=16, batch_size=128, lr=2e-3, seed=0,
        device="cuda:0", verbose=True, deterministic=False, recompute=False, stack=1, device_optimizer=False):
    torch.manual_seed(seed)      # (already seeds the parameters and the dropout masks; deterministic=True makes the gradients repeat too)
    feat_dim = 129 if schema == "mag" else 256
    batches = []
    for b in range(4 * stack):      # a small pool of sampled batches, cycled like an epoch of pre-sampled jobs (train_ogbn_mag.py:82-104)
        fe, ti, el, graph = synthetic_sampled_batch(schema, n_seed=batch_size, width=64, depth=4, feat_dim=feat_dim, mean_degree=6.0,
                                                    seed=seed * 100 + b)
        dg = to_device_graph(fe, ti, el, graph, device=device, plan=stack == 1)      # pieces that are only stacked need no plan
        g = torch.Generator().manual_seed(b)
        proj = torch.randn(feat_dim, n_classes, generator=g)
        labels = (dg[0][:batch_size].cpu() @ proj).argmax(dim=1).to(device)     # a learnable synthetic task on the seed papers
        batches.append((dg, labels, slice(0, batch_size)))
    if stack > 1:          # B batches -> one graph; its seed rows are the pieces' first batch_size papers
        groups = [batches[i:i + stack] for i in range(0, len(batches), stack)]
        batches = []
        for grp in groups:
            sg = stack_device_graphs([dg for dg, _, _ in grp])
            batches.append((sg, torch.cat([y for _, y, _ in grp]), torch.cat([sg.rows(b, "paper", range(batch_size)) for b in range(len(grp))])))
    T, R = len(batches[0][0][5]), len(batches[0][0][6])
    gnn = GNN(feat_dim, n_hid, T, R, n_heads, n_layers, dropout=0.2, conv_name=conv, prev_norm=True, last_norm=True, use_RTE=True).to(device)
    head = Classifier(n_hid, n_classes).to(device)
    if recompute:          # memory-lean: the layers keep neither Q|K|V, the a_linear output nor the dropout masks for the backward
        import pyhgt_amd
        pyhgt_amd.set_recompute(gnn, True)
    if deterministic:      # every reduction of the backward in a fixed order: two runs with one seed give the same bits
        import pyhgt_amd
        pyhgt_amd.set_deterministic(gnn, True), pyhgt_amd.set_deterministic(head, True)
    if device_optimizer:   # clip + AdamW in three launches of pyhgt_amd's own kernels; the head stays out of the norm, as below
        import pyhgt_amd
        opt = pyhgt_amd.AdamW([dict(params=list(gnn.parameters())), dict(params=list(head.parameters()), clip=False)], lr=lr, max_norm=0.5)
    else:
        opt = torch.optim.AdamW(list(gnn.parameters()) + list(head.parameters()), lr=lr)
    losses, t0 = [], time.perf_counter()
    for step in range(steps):
        (x, nt, tm, ei, et, _, _), y, seeds = batches[step % len(batches)]
        gnn.train(), head.train()
        rep = gnn(x, nt, tm, ei, et)
        loss = torch.nn.functional.nll_loss(head(rep[seeds]), y)
        opt.zero_grad()
        loss.backward()
        if not device_optimizer:
            torch.nn.utils.clip_grad_norm_(gnn.parameters(), 0.5)
        opt.step()
        losses.append(loss.item())
        if verbose and (step % 5 == 0 or step == steps - 1):
            print("step %3d  loss %.4f" % (step, losses[-1]))
    torch.cuda.synchronize()
    if verbose:
        print("%.1f ms per training step (%d nodes, %d edges, %d layers, conv=%s)" % ((time.perf_counter() - t0) / steps * 1e3, nt.numel(),
                                                                                   et.numel(), n_layers, conv))
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--schema", default="mag", choices=["mag", "oag"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--conv", default="hgt", choices=["hgt", "dense_hgt"])
    ap.add_argument("--n-hid", type=int, default=int(os.environ.get("HGT_TRAIN_D", 128)), help="hidden width (e.g. 768 with 8 heads)")
    ap.add_argument("--n-heads", type=int, default=int(os.environ.get("HGT_TRAIN_H", 8)))
    ap.add_argument("--deterministic", action="store_true", help="bit-reproducible training: atomic-free backward, torch seeded with --seed")
    ap.add_argument("--recompute", action="store_true", help="memory-lean training: Q|K|V and the dropout masks are recomputed in the backward")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--stack", type=int, default=1, help="sampled batches per optimizer step, stacked on the device into one graph")
    ap.add_argument("--device-optimizer", action="store_true", help="pyhgt_amd.AdamW(max_norm=0.5) in place of clip_grad_norm_ + torch.optim.AdamW")
    a = ap.parse_args()
    run(a.schema, a.steps, a.conv, n_hid=a.n_hid, n_heads=a.n_heads, seed=a.seed, deterministic=a.deterministic, recompute=a.recompute, stack=a.stack,
        device_optimizer=a.device_optimizer)
