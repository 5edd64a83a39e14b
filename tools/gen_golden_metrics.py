"""Fixtures of the task metrics: tests/golden/task/metrics_small.npz.

    python tools/gen_golden_metrics.py          (needs the reference tree: oracle.reference_loader.load_reference_data())

The reference's scripts score a batch one row at a time (OAG/train_paper_field.py:272-275): the labels of a row are put into the order
of `argsort(descending=True)` of its scores and handed to the verbatim `ndcg_at_k` and `mean_reciprocal_rank` (pyHGT/utils.py:5-20,
which pyHGT/data.py star-imports).  This script does exactly that on fixed small rows and records the inputs and the two results per
row.  The scores of a row come from a permutation, so they are distinct (asserted; plain float32 normals at C = 3000 do collide) and
the reference's unstable argsort has one answer.  It also records the pair-ranking loss `mask_softmax`
(OAG/train_author_disambiguation.py:90-96), restated below and evaluated in float64 with its gradient.  The file sits in a
sub-directory because tests/conftest.py takes tests/golden/*.npz for layer fixtures.  tests/test_task_metrics.py imports the helpers.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "task", "metrics_small.npz")

# (C, P, graded): P positives among C positions; graded = relevances of several sizes instead of the paper-field 1 / P
CASES = [(1, 0, False), (1, 1, False), (2, 1, False), (3, 2, True), (5, 5, False), (17, 3, True), (63, 1, False), (64, 7, False),
         (65, 64, True), (100, 0, False), (257, 1, False), (257, 256, False), (1000, 7, True), (1000, 999, False), (3000, 1, False),
         (3000, 40, True), (3000, 1500, False), (4099, 1023, False), (4099, 1025, True), (5000, 4096, False)]
LOSS_SIZES = [2, 3, 4, 6, 10, 63, 64, 65, 300, 4, 4, 5]


def make_rows(seed=0):
    """-> (scores flat float32, labels flat float32, sizes, k per row; 0 = None): every case twice, with k = C and with k = C // 3"""
    rng = np.random.default_rng(seed)
    scores, labels, sizes, ks = [], [], [], []
    for C, P, graded in CASES:
        for k in [0] + ([C // 3] if C >= 3 else []):
            s = ((rng.permutation(C) - C / 2.0) * 0.0078125).astype(np.float32)            # multiples of 2^-7: exact and distinct
            assert np.unique(s).size == C
            l = np.zeros(C, np.float32)
            where = rng.choice(C, size=P, replace=False)
            l[where] = rng.integers(1, 5, size=P).astype(np.float32) / 4 if graded else np.float32(1.0 / max(P, 1))
            scores.append(s), labels.append(l), sizes.append(C), ks.append(k)
    return np.concatenate(scores), np.concatenate(labels), np.asarray(sizes, np.int64), np.asarray(ks, np.int64)


def reference_rows(data, scores, labels, sizes, ks):
    """the script's procedure per row -> (ndcg, mrr) float64"""
    ndcg, mrr, beg = [], [], 0
    for C, k in zip(sizes.tolist(), ks.tolist()):
        s, l = torch.from_numpy(scores[beg:beg + C]), torch.from_numpy(labels[beg:beg + C])
        r = l[s.argsort(descending=True)].tolist()
        ndcg.append(data.ndcg_at_k(r, k if k else len(r)))
        mrr.append(data.mean_reciprocal_rank([r])[0])
        beg += C
    return np.asarray(ndcg, np.float64), np.asarray(mrr, np.float64)


def mask_softmax64(pred, size):
    """mask_softmax of the script, restated, on a float64 tensor"""
    loss, stx = 0, 0
    for l in size:
        loss = loss + torch.log_softmax(pred[stx:stx + l], dim=-1)[0] / np.log(l)
        stx += l
    return -loss


def main():
    from oracle.reference_loader import load_reference_data
    data = load_reference_data()
    scores, labels, sizes, ks = make_rows()
    ndcg, mrr = reference_rows(data, scores, labels, sizes, ks)
    rng = np.random.default_rng(1)
    x = (rng.uniform(-30, 30, size=sum(LOSS_SIZES))).astype(np.float32)
    x[LOSS_SIZES[0] + LOSS_SIZES[1] + 1] = 80.0                                   # a dominant entry in the third segment
    x64 = torch.from_numpy(x).double().requires_grad_()
    loss = mask_softmax64(x64, LOSS_SIZES)
    loss.backward()
    blob = {"rank/scores": scores, "rank/labels": labels, "rank/sizes": sizes, "rank/k": ks, "rank/ndcg": ndcg, "rank/mrr": mrr,
            "loss/scores": x, "loss/sizes": np.asarray(LOSS_SIZES, np.int64), "loss/value": np.float64(loss.item()),
            "loss/grad": x64.grad.numpy()}
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **blob)
    print(len(sizes), "rows,", int(sizes.sum()), "positions; largest P", int(max((labels[b:b + c] > 0).sum() for b, c in
          zip(np.concatenate([[0], np.cumsum(sizes)[:-1]]), sizes))), "; loss", loss.item())
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
