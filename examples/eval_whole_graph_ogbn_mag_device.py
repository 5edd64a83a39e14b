#!/usr/bin/env python
"""Exact evaluation on the whole resident graph, next to the voted, sampled evaluation of eval_ogbn_mag.py.

The task, the graph and the training loop are those of examples/train_eval_ogbn_mag_device.py (imported, not copied): a few sampled
training steps, then the voted evaluation of the test papers in both modes of the script.  Then the same model on
`dgraph.whole_graph(node_time=...)`, the resident graph as it is:

  voted     eval_ogbn_mag.py:128-191 -- sub-graphs around chunks of test papers, log-probabilities summed per paper (as before)
  exact     ONE forward over all nodes and edges and one Classifier.predict(rep, ids=arange, labels=y, split=split, n_splits=3): the
            train / valid / test accuracies of every paper in one pass, no sampling, nothing to vote on
  chunk     the exact output of one chunk of test papers through `seeds=`: each layer computes only the rows those papers need

    python examples/eval_whole_graph_ogbn_mag_device.py [--steps 30] [--papers 20000]

The layers use the temporal encoding, so every node needs a time.  A paper has its year.  WHICH time another node gets on a whole graph
is the caller's decision -- the reference knows such times per sampled batch only (data.py:125) -- and this example decides: the latest
stored time among the node's entries (an author's latest paper), the graph's last year where it has none."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_eval_ogbn_mag_device as E  # noqa: E402
from pyhgt_amd.sampler import TIME_NONE  # noqa: E402


def node_times(dgraph, year, default):
    """{type: int32 device tensor}: the papers' years; another node's latest stored entry time, `default` where it has none"""
    dev = dgraph.device
    latest = {t: torch.full((n,), TIME_NONE, dtype=torch.int32, device=dev) for t, n in zip(dgraph.types, dgraph.n_nodes)}
    for (tt, _, _), (ip, _, tm) in zip(dgraph.triples, dgraph.csr_dev):
        if tm.numel():                                           # (TIME_NONE is the smallest int32: it never wins the maximum)
            row = torch.repeat_interleave(torch.arange(ip.numel() - 1, device=dev), (ip[1:] - ip[:-1]).long(), output_size=tm.numel())
            latest[tt].scatter_reduce_(0, row, tm, "amax")
    times = {t: torch.where(v != TIME_NONE, v, torch.full_like(v, int(default))) for t, v in latest.items()}
    times["paper"] = torch.as_tensor(year, dtype=torch.int32).to(dev)
    return times


def _trained(steps, n_paper, n_classes, seed, device, verbose, **kw):
    """the training loop and the voted evaluation of train_eval_ogbn_mag_device.run, with the model it built handed back.
    `run` returns neither the model nor the graph and that file stays as it is, so its `GNN` / `Classifier` names are swapped for
    recording factories while it runs (restored in `finally`; not for concurrent callers of that module), and the caller rebuilds the
    graph with the same `task_graph` arguments -- a pure function of them.  A hook in `run` would replace both."""
    built = {}

    def keep(cls, name):
        def make(*a, **k):
            built[name] = cls(*a, **k)
            return built[name]
        return make

    gnn_cls, head_cls = E.GNN, E.Classifier
    E.GNN, E.Classifier = keep(gnn_cls, "gnn"), keep(head_cls, "head")
    try:
        losses, accs, tables = E.run(steps, n_paper, n_classes, seed=seed, device=device, verbose=verbose, **kw)
    finally:
        E.GNN, E.Classifier = gnn_cls, head_cls
    return built["gnn"], built["head"], losses, tables


def run(steps=30, n_paper=20000, n_classes=349, batch_size=128, seed=0, device="cuda:0", verbose=True, feat_dim=129, **kw):
    """-> dict(voted={mode: accuracy}, exact=dict(counts=[[n, correct]] per split, accuracy=[...], logits, y, split), chunk=dict(ids,
    seeds_out, whole_out), losses).  The tensors are on the device; kw goes to train_eval_ogbn_mag_device.run (n_hid, n_layers, ...)."""
    gnn, head, losses, tables = _trained(steps, n_paper, n_classes, seed, device, verbose, batch_size=batch_size, feat_dim=feat_dim, **kw)
    dgraph, n_nodes, year, y_host, split_host = E.task_graph(n_paper, feat_dim, n_classes, device, seed)      # the same graph again
    y, split = torch.from_numpy(y_host).to(device), torch.from_numpy(split_host).to(device)
    test_paper = np.flatnonzero(split_host == 2)
    np.random.default_rng(43).shuffle(test_paper)
    y_test = y[torch.from_numpy(test_paper).to(device)]
    voted = {mode: table.accuracy(y_test) for mode, table in tables.items()}
    gnn.eval(), head.eval()
    view = dgraph.whole_graph(node_time=node_times(dgraph, year, E.YEARS[1] - 1))
    with torch.no_grad():
        rep = gnn(*view[:5])[view.type_rows("paper")]
        ids = torch.arange(n_nodes["paper"], device=device)
        counts = head.predict(rep, ids=ids, labels=y, split=split, n_splits=3)[1].tolist()
        logits = head.logits(rep)
        chunk = torch.from_numpy(test_paper[:batch_size]).to(device)
        seeds_out = gnn(*view[:5], seeds=view.rows("paper", chunk))
    exact = [c / n if n else float("nan") for n, c in counts]
    if verbose:
        print("whole graph: %d nodes, %d edges" % (view[1].numel(), view[3].size(1)))
        print("test accuracy  voted variance_reduce %.3f | voted sequential %.3f | exact (one forward) %.3f"
              % (voted["variance_reduce"], voted["sequential"], exact[2]))
        print("exact accuracy of every paper in the same pass: train %.3f (%d papers)  valid %.3f (%d)  test %.3f (%d)"
              % (exact[0], counts[0][0], exact[1], counts[1][0], exact[2], counts[2][0]))
        print("exact inference of %d test papers through seeds=: max |difference from the whole forward| %.2e"
              % (chunk.numel(), (seeds_out - rep[chunk]).abs().max().item()))
    return dict(voted=voted, exact=dict(counts=counts, accuracy=exact, logits=logits, y=y, split=split),
                chunk=dict(ids=chunk, seeds_out=seeds_out, whole_out=rep[chunk]), losses=losses,
                precision=gnn.gcs[0].base_conv.precision)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--papers", type=int, default=20000)
    ap.add_argument("--classes", type=int, default=349)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    run(a.steps, a.papers, a.classes, seed=a.seed)
