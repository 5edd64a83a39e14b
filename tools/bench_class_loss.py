#!/usr/bin/env python
"""The classification losses: torch's chain against the device calls of pyhgt_amd/metrics.py, forward and backward, on the same tensors.

    python tools/bench_class_loss.py [--reps 15] [--out profiles/r15_class_loss.json]

Torch side, as the training scripts and Classifier.forward under autograd do it: torch.log_softmax on the logits, then nll_loss
(OAG/train_paper_venue.py:86, ogbn-mag/train_ogbn_mag.py:116) or KLDivLoss(reduction='batchmean') (OAG/train_paper_field.py:87),
and backward to the logits.  Device side: class_loss and its backward.  The last case builds the labels inside the timed window on both
sides: LabelSpace.distribution (dense [n, C]) for torch, LabelSpace.columns (width 8) for the device.  Both sides of a case run
alternately in this process after a warm-up; every time is a host clock around work that ends in a device synchronise, and the figure
reported is the median over --reps repetitions.  No time is asserted."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import DeviceHeteroGraph, LabelSpace, class_loss  # noqa: E402


def alternate(sides, reps, warmup=3):
    """sides = {name: callable}; -> {name: median ms}, the callables run in turn and each ends synchronised"""
    times, last = {k: [] for k in sides}, {}
    for i in range(warmup + reps):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}, last


def field_graph(n_paper, n_field, per_paper, device, seed=3):
    """papers with `per_paper` distinct fields each: the one relation the label kernels read"""
    rng = np.random.default_rng(seed)
    src = np.stack([rng.choice(n_field, per_paper, replace=False) for _ in range(n_paper)]).reshape(-1)
    indptr = np.arange(n_paper + 1) * per_paper
    feats = {"paper": np.zeros((n_paper, 1), np.float32), "field": np.zeros((n_field, 1), np.float32)}
    return DeviceHeteroGraph.from_csr(["paper", "field"], [("paper", "field", "PF")], {"paper": n_paper, "field": n_field},
                                      [(indptr, src, np.full(src.size, 2010))], feats, device=device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "r15_class_loss.json"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("medians of at least 10")
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to time without one"
    dev, rng = "cuda:0", np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
              "unit": "ms, median, host clock around forward + backward ending in a device synchronise", "cases": []}

    def record(what, n, c, sides, tol):
        ms, last = alternate(sides, a.reps)
        got, want = last["device"], last["torch"]
        assert abs(got[0] - want[0]) <= tol * max(1.0, abs(want[0])), (got[0], want[0])
        assert (got[1] - want[1]).abs().max().item() <= 1e-6, "gradients differ"
        result["cases"].append({"what": what, "rows": n, "C": c, **ms})
        print(result["cases"][-1], flush=True)

    def step(x, loss_of):
        leaf = x.detach().requires_grad_()
        loss = loss_of(leaf)
        loss.backward()
        return loss.item(), leaf.grad

    for n, c in ((256, 349), (256, 1000)):
        x = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32) * 3).to(dev)
        y = torch.from_numpy(rng.integers(0, c, size=n)).to(dev)
        record("log_softmax + nll_loss, index", n, c,
               {"torch": lambda: step(x, lambda t: torch.nn.functional.nll_loss(torch.log_softmax(t, dim=-1), y)),
                "device": lambda: step(x, lambda t: class_loss(t, index=y))}, 1e-5)

    n, c, per_paper = 256, 20000, 5
    g = field_graph(4096, c, per_paper, dev)
    space = LabelSpace(g, ("paper", "field", "PF"), np.arange(c))
    papers = torch.from_numpy(rng.choice(4096, n, replace=False)).to(dev)
    x = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32) * 3).to(dev)
    dense = space.distribution(papers)
    kl = torch.nn.KLDivLoss(reduction="batchmean")
    record("log_softmax + KLDivLoss, dense labels", n, c,
           {"torch": lambda: step(x, lambda t: kl(torch.log_softmax(t, dim=-1), dense)),
            "device": lambda: step(x, lambda t: class_loss(t, labels=dense))}, 1e-5)
    record("labels + log_softmax + KLDivLoss: distribution against columns of width 8", n, c,
           {"torch": lambda: step(x, lambda t: kl(torch.log_softmax(t, dim=-1), space.distribution(papers))),
            "device": lambda: step(x, lambda t: class_loss(t, **dict(zip(("columns", "count"), space.columns(papers, width=8)))))}, 1e-5)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
