#!/usr/bin/env python
"""Training on a destination partition: every rank owns a contiguous range of target nodes and all their in-edges, keeps the
remote sources as halo rows, and per layer exchanges features forward and halo gradients backward (pyhgt_amd/dist.py).

    python -m torch.distributed.run --standalone --nproc-per-node W examples/train_partitioned.py [--backend gloo|nccl]
           [--device-index I] [--steps 20] [--nodes 6000] [--edges 60000] [--n-hid 64] [--n-heads 4] [--deterministic]

--device-index puts every rank on ONE device (with --backend gloo: the collectives are staged through the host), so the multi-rank
path runs on a single GPU; without it rank r uses device r (nccl = RCCL).  A synthetic global graph goes through `partition` and
`PartitionedGraph`, then two HGTConv layers chained by hand and a linear head on the rank's own rows:
loss -> backward -> all_reduce_grads -> AdamW.  The loss is the sum over the rank's rows divided by the GLOBAL node count, so the
all-reduced gradient is that of the global mean and every rank takes the same optimizer step."""
import argparse
import datetime
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import HGTConv, set_deterministic  # noqa: E402
from pyhgt_amd.dist import PartitionedGraph, all_reduce_grads, partition  # noqa: E402
from pyhgt_amd.synth import synthetic_typed_graph  # noqa: E402


def run(backend="gloo", device_index=None, steps=20, nodes=6000, edges=60000, n_hid=64, n_heads=4, n_classes=8, lr=5e-3, seed=0,
        deterministic=False, align=256):
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = torch.device("cuda", rank % torch.cuda.device_count() if device_index is None else device_index)
    torch.cuda.set_device(dev)
    T, R = 3, 4
    # every rank draws the same global graph and cuts its share out of it (a real run would load its share only)
    x, nt, ei, et, tm = synthetic_typed_graph(nodes, edges, n_hid, T, R, seed=seed, sorted_types=False)
    g = torch.Generator().manual_seed(seed + 1)
    labels = (x @ torch.randn(n_hid, n_classes, generator=g)).argmax(dim=1)          # a learnable synthetic task
    part = partition(nt, ei, et, tm, world, rank, align=align)
    offsets = part["node_offsets"]
    lo, hi = offsets[rank], offsets[rank + 1]
    if any(offsets[r + 1] <= offsets[r] for r in range(world)):      # (every rank sees the same offsets: all of them stop here)
        raise SystemExit("the partition leaves a rank without targets (offsets %s): use fewer ranks" % offsets)
    pg = PartitionedGraph(part["node_type_own"].to(dev), part["src_global"].to(dev), part["dst_local"].to(dev), part["edge_type"].to(dev),
                          part["edge_time"].to(dev), T, R, 0, rank, world, node_offsets=offsets)
    torch.manual_seed(seed)            # the same initial parameters on every rank
    layers = torch.nn.ModuleList([HGTConv(n_hid, n_hid, T, R, n_heads, dropout=0.2) for _ in range(2)]).to(dev)
    head = torch.nn.Linear(n_hid, n_classes).to(dev)
    model = torch.nn.ModuleList([layers, head])
    if deterministic:                  # this rank's gradients repeat bit for bit; the all-reduce is the collective library's business
        set_deterministic(model, True)
    torch.manual_seed(seed + 100 + rank)      # ... and different dropout masks
    opt = torch.optim.AdamW(model.parameters(), lr=lr)
    x_own, y_own = x[lo:hi].to(dev), labels[lo:hi].to(dev)
    losses = []
    for step in range(steps):
        model.train()
        h = x_own
        for layer in layers:           # the output of one partitioned layer is the x_own of the next
            h = pg.forward(layer, h)
        loss = torch.nn.functional.cross_entropy(head(h), y_own, reduction="sum") / nodes
        opt.zero_grad()
        loss.backward()
        all_reduce_grads(model)
        opt.step()
        total = loss.detach().clone()
        if backend == "gloo":
            total = total.cpu()
        dist.all_reduce(total)         # the global mean loss, the same number on every rank
        losses.append(float(loss.detach()))
        # (one write per line: the ranks share the launcher's stdout)
        sys.stdout.write("rank %d step %3d loss %.5f global %.5f (own rows %d, halo rows %d)\n" % (rank, step, losses[-1], float(total), pg.n_own,
                                                                                                  pg.n_local - pg.n_own))
        sys.stdout.flush()
    torch.cuda.synchronize()
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="gloo", choices=["gloo", "nccl"])
    ap.add_argument("--device-index", type=int, default=None, help="put every rank on this device (one GPU plays all ranks)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=6000)
    ap.add_argument("--edges", type=int, default=60000)
    ap.add_argument("--n-hid", type=int, default=64)
    ap.add_argument("--n-heads", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true")
    a = ap.parse_args()
    dist.init_process_group(a.backend, timeout=datetime.timedelta(seconds=120))
    try:
        run(a.backend, a.device_index, a.steps, a.nodes, a.edges, a.n_hid, a.n_heads, seed=a.seed, deterministic=a.deterministic)
    finally:
        dist.destroy_process_group()
