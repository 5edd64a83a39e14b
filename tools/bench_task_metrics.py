#!/usr/bin/env python
"""Scoring a task batch: the host loop of the reference's scripts against the device calls of pyhgt_amd/metrics.py, on the same tensors.

    python tools/bench_task_metrics.py [--reps 15] [--out profiles/r14_task_metrics.json]

Host side, restated from the scripts: the metrics take `argsort(descending=True)` of the scores, then per row the labels in that order
are copied to the host and turned into a list, and DCG / ideal DCG / the first non-zero position are computed with numpy on it
(OAG/train_paper_field.py:303-308, train_author_disambiguation.py:335-345); the loss is one log_softmax per segment
(train_author_disambiguation.py:90-96), forward and backward.  Device side: rank_metrics / pair_rank_loss, ending in one scalar each.
Both sides of a case run alternately in this process after a warm-up; every time is a host clock around work that ends in a device
synchronise, and the figure reported is the median over --reps repetitions."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import Segments, pair_rank_loss, rank_metrics  # noqa: E402


def _dcg(r):
    r = np.asarray(r, dtype=np.float64)
    return float(r[0] + np.sum(r[1:] / np.log2(np.arange(2, r.size + 1)))) if r.size else 0.0


def host_rows(scores, labels):
    """per row: the labels in argsort order -> host list -> NDCG and reciprocal rank"""
    ndcg, rr = [], []
    for l, order in zip(labels, scores.argsort(descending=True)):
        r = l[order].cpu().numpy().tolist()
        best = _dcg(sorted(r, reverse=True))
        ndcg.append(_dcg(r) / best if best else 0.0)
        hit = np.asarray(r).nonzero()[0]
        rr.append(1.0 / (hit[0] + 1) if hit.size else 0.0)
    return float(np.mean(ndcg)), float(np.mean(rr))


def host_segments(res, sizes):
    ndcg, rr, beg = [], [], 0
    for s in sizes:
        l = torch.zeros(s)
        l[0] = 1
        r = l[res[beg:beg + s].argsort(descending=True).cpu()].tolist()
        ndcg.append(_dcg(r) / _dcg(sorted(r, reverse=True)))
        rr.append(1.0 / (np.asarray(r).nonzero()[0][0] + 1))
        beg += s
    return float(np.mean(ndcg)), float(np.mean(rr))


def host_loss(pred, sizes):
    loss, beg = 0, 0
    for l in sizes:
        loss = loss + torch.log_softmax(pred[beg:beg + l], dim=-1)[0] / np.log(l)
        beg += l
    return -loss


def alternate(sides, reps, warmup=3):
    """sides = {name: callable}; -> {name: median ms}, the callables run in turn and each ends synchronised"""
    times = {k: [] for k in sides}
    for i in range(warmup + reps):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "r14_task_metrics.json"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("medians of at least 10")
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to time without one"
    dev, rng = "cuda:0", np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "unit": "ms, median, host clock around a synchronised call",
              "cases": []}
    for n, c in ((256, 1000), (256, 20000)):
        # distinct within a row (a permutation), so that the unstable argsort of the host side has one answer
        scores = torch.from_numpy((rng.permuted(np.tile(np.arange(c), (n, 1)), axis=1) * 0.001).astype(np.float32)).to(dev)
        lab = (rng.random((n, c)) < 5.0 / c).astype(np.float32)
        lab /= np.maximum(lab.sum(1, keepdims=True), 1)
        labels = torch.from_numpy(lab).to(dev)

        def device_side():
            ndcg, rr = rank_metrics(scores, labels=labels)
            return ndcg.mean().item(), rr.mean().item()

        ms, got = alternate({"host_loop": lambda: host_rows(scores, labels), "device": device_side}, a.reps)
        want = host_rows(scores, labels)
        assert abs(got[0] - want[0]) < 1e-9 and abs(got[1] - want[1]) < 1e-9, (got, want)
        result["cases"].append({"what": "NDCG and MRR, dense labels", "rows": n, "C": c, **ms})
        print(result["cases"][-1], flush=True)

    sizes = [6] * 256
    res = torch.from_numpy((rng.permutation(sum(sizes)) * 0.01 - 7.0).astype(np.float32)).to(dev)
    seg = Segments(sizes, dev)

    def device_segments():
        ndcg, rr = rank_metrics(res, sizes=seg)
        return ndcg.mean().item(), rr.mean().item()

    ms, got = alternate({"host_loop": lambda: host_segments(res, sizes), "device": device_segments}, a.reps)
    want = host_segments(res, sizes)
    assert abs(got[0] - want[0]) < 1e-9 and abs(got[1] - want[1]) < 1e-9, (got, want)
    result["cases"].append({"what": "NDCG and MRR, author segments", "segments": len(sizes), "length": 6, **ms})
    print(result["cases"][-1], flush=True)

    def torch_loss():
        x = res.clone().requires_grad_()
        loss = host_loss(x, sizes)
        loss.backward()
        return loss.item()

    def device_loss():
        x = res.clone().requires_grad_()
        loss = pair_rank_loss(x, seg)
        loss.backward()
        return loss.item()

    ms, got = alternate({"log_softmax_loop": torch_loss, "device": device_loss}, a.reps)
    want = torch_loss()
    assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (got, want)
    result["cases"].append({"what": "pair-ranking loss, forward and backward", "segments": len(sizes), "length": 6, **ms})
    print(result["cases"][-1], flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
