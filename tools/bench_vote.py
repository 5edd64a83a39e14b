#!/usr/bin/env python
"""The voted evaluation of ogbn-mag/eval_ogbn_mag.py three ways on the same tensors: the script's host loop, torch's device chain and
the device path of pyhgt_amd/metrics.py (VoteTable).

    python tools/bench_vote.py [--reps 15] [--out profiles/r16_vote_eval.json]

A case is one variance_reduce round of the script: B sub-graphs (pieces) whose paper rows went through the Classifier, the raw logits
[rows, C] of all of them, the paper id of every row, and a table with one slot per test paper.  The first 128 ids of every piece are the
same test papers (the seeds); the others are distinct random papers, of which the test share has a slot.  Timed, table reset included:
  host     the script: per piece log_softmax of the test-masked rows, `res.tolist()`, `y_preds[pi] += r` in a dict of numpy vectors;
           then the argmax of every vector against its label (eval_ogbn_mag.py:148-150, 182-190)
  torch    on the device: log_softmax -> index_add_ into the table (rows without a slot go to a spare row, so nothing synchronises;
           the adds are float atomics) -> argmax -> masked compares, one host read of (voted, correct)
  device   VoteTable.add(logits, ids, piece_sizes) -> VoteTable.accuracy(labels): one launch per piece, no atomics, one launch for the
           answer, one host read
The three run alternately in this process after a warm-up; every time is a host clock around work that ends in a device synchronise
(or on the host), and the figure reported is the median over --reps repetitions.  No time is asserted; the three answers are."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import VoteTable  # noqa: E402


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


def make_case(rng, n_nodes, n_slots, n_classes, pieces, rows, n_seed, dev):
    """-> (logits [pieces * rows, C], ids, piece sizes, test nodes, labels per slot, the host's view of it)"""
    test = rng.permutation(n_nodes)[:n_slots]
    seeds = test[:n_seed]
    rest = np.setdiff1d(np.arange(n_nodes), seeds)
    ids = np.concatenate([np.concatenate([seeds, rng.choice(rest, rows - n_seed, replace=False)]) for _ in range(pieces)])
    y = rng.integers(0, n_classes, size=n_nodes)
    x = rng.standard_normal((ids.size, n_classes)).astype(np.float32)
    x[np.arange(ids.size), y[ids]] += 2.0                                          # a signal: the vote is mostly right
    return (torch.from_numpy(x).to(dev), torch.from_numpy(ids).to(dev), [rows] * pieces, test, torch.from_numpy(y[test]).to(dev),
            dict(ids=ids, y=y, test=test))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("profiles", "r16_vote_eval.json"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("medians of at least 10")
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to time without one"
    dev, rng = "cuda:0", np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
              "unit": "ms, median, host clock around reset + votes + answer, ending in a device synchronise", "cases": []}

    for what, n_nodes, n_slots, c, pieces, rows, n_seed in (
            ("ogbn-mag variance_reduce round: 8 pieces of 3250 paper rows", 736389, 41939, 349, 8, 3250, 128),
            ("one piece of 128 rows", 736389, 41939, 349, 1, 128, 128),
            ("one piece of 256 rows, 20000 classes", 65536, 4096, 20000, 1, 256, 128)):
        x, ids, sizes, test, labels, H = make_case(rng, n_nodes, n_slots, c, pieces, rows, n_seed, dev)
        test_mask = np.zeros(n_nodes, bool)
        test_mask[test] = True
        masks = [torch.from_numpy(test_mask[H["ids"][b * rows:(b + 1) * rows]]).to(dev) for b in range(pieces)]
        yindxs = [H["ids"][b * rows:(b + 1) * rows][test_mask[H["ids"][b * rows:(b + 1) * rows]]].tolist() for b in range(pieces)]

        def host():
            y_preds = {pi: np.zeros(c) for pi in test.tolist()}
            voted = set()
            for b in range(pieces):
                res = torch.log_softmax(x[b * rows:(b + 1) * rows][masks[b]], dim=-1)
                for pi, r in zip(yindxs[b], res.tolist()):
                    y_preds[pi] += r
                    voted.add(pi)
            correct = sum(int(y_preds[pi].argmax() == H["y"][pi]) for pi in voted)
            return len(voted), correct

        table = VoteTable(n_nodes, c, nodes=test, device=dev)
        votes = torch.zeros(n_slots + 1, c, device=dev)                             # torch's table: a spare row for the rows without a slot
        count = torch.zeros(n_slots + 1, dtype=torch.int32, device=dev)
        ones = torch.ones(ids.numel(), dtype=torch.int32, device=dev)
        slot_of = table.slot_of.long()

        def chain():
            votes.zero_(), count.zero_()
            slot = slot_of[ids]
            slot = torch.where(slot >= 0, slot, n_slots)
            votes.index_add_(0, slot, torch.log_softmax(x, dim=-1))
            count.index_add_(0, slot, ones)
            pred, voted = votes[:n_slots].argmax(dim=1), count[:n_slots] > 0
            return tuple(torch.stack([voted.sum(), (voted & (pred == labels)).sum()]).tolist())

        def device():
            table.reset()
            table.add(x, ids, piece_sizes=sizes)
            return tuple(table.predict(labels)[1].tolist())

        ms, last = alternate({"host": host, "torch": chain, "device": device}, a.reps)
        assert last["host"][0] == last["torch"][0] == last["device"][0], last
        assert max(abs(last[k][1] - last["host"][1]) for k in ("torch", "device")) <= 0.01 * last["host"][0], last
        result["cases"].append({"what": what, "pieces": pieces, "rows_per_piece": rows, "C": c, "slots": n_slots, "voted": last["device"][0],
                                "correct": last["device"][1], **ms})
        print(result["cases"][-1], flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
