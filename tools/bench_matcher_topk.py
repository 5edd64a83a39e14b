#!/usr/bin/env python
"""Matcher retrieval against the dense chain, one setting per process:

    python tools/bench_matcher_topk.py --only SETTING [--repeats 5] [--out profiles/r23_matcher_topk.json] [--kernels-only]

  n{N}_q{Q}_h{H}   N in 100 000, 1 000 000, 4 000 000 candidates, Q in 1, 16, 256 queries, n_hid H in 256, 400; random normal embeddings,
                   a Matcher with its default initialisation, the candidates projected once into the Matcher's cache (infer=True) before
                   anything is timed, so both sides start from the same cached [N, H] tensor and project the Q queries inside the clock:
                     topk_k10 / topk_k100      Matcher.topk(x, y, k, infer=True)
                     dense_topk_k10 / _k100    torch.topk(Matcher.forward(x, y, infer=True).t(), k): the [N, Q] matrix, then a selection
                     rank_of                   Matcher.rank_of(x, y, index, infer=True)
                     dense_rank                the [N, Q] matrix, then (s > s_t).sum + ((s == s_t) & (c < t)).sum over it
                   each with the peak device allocation of one call above what was allocated before it, and whether the two sides'
                   answers agree (indices where the dense scores have no tie within float32 rounding; ranks within the same room).

A host clock around each call, which ends in a synchronise; after a warm-up call, the median, minimum and maximum over `repeats` calls.
--kernels-only runs three calls of topk (k = 10, 100) and rank_of and nothing else: the process to put under a kernel trace.
--out merges the setting into the JSON file, so the processes fill one file."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import Matcher  # noqa: E402

DEV = "cuda:0"
SETTINGS = ["n%d_q%d_h%d" % (n, q, h) for h in (256, 400) for n in (100000, 1000000, 4000000) for q in (1, 16, 256)]


def stats(v, digits=3):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits), "n": len(v)}


def timed(fn, repeats, warmup=1):
    out = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
        del res
    return out


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del res
    return round(peak / 2 ** 20, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", required=True, choices=SETTINGS)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, Q, H = (int(v[1:]) for v in a.only.split("_"))
    torch.manual_seed(0)
    m = Matcher(H).to(DEV).eval()
    x = torch.randn(N, H, device=DEV)
    y = torch.randn(Q, H, device=DEV)
    index = torch.randint(0, N, (Q,), device=DEV)
    cols = torch.arange(Q, device=DEV)
    pos = torch.arange(N, device=DEV)[:, None]
    row = {"n_cand": N, "n_query": Q, "n_hid": H, "device_name": torch.cuda.get_device_name(0), "dense_matrix_mib": round(N * Q * 4 / 2 ** 20, 2),
           "floor_stream_us": round(N * H * 4 / 7.2e12 * 1e6, 1), "floor_fp32_matrix_us": round(2.0 * N * Q * H / 155e12 * 1e6, 1)}

    def dense_topk(k):
        return torch.topk(m(x, y, infer=True).t(), k)

    def dense_rank():
        s = m(x, y, infer=True)
        st = s[index, cols]
        return (s > st).sum(0) + ((s == st) & (pos < index)).sum(0)

    with torch.no_grad():
        m.topk(x, y, 10, infer=True)                                  # fills the cache: nothing below projects the candidates
        if a.kernels_only:
            for _ in range(3):
                m.topk(x, y, 10, infer=True)
                m.topk(x, y, 100, infer=True)
                m.rank_of(x, y, index, infer=True)
            torch.cuda.synchronize()
            print(a.only, "kernels only: done", flush=True)
            return
        for k in (10, 100):
            row["topk_k%d_ms" % k] = stats(timed(lambda: m.topk(x, y, k, infer=True), a.repeats))
            row["dense_topk_k%d_ms" % k] = stats(timed(lambda: dense_topk(k), a.repeats))
            row["topk_k%d_peak_mib" % k] = peak_mib(lambda: m.topk(x, y, k, infer=True))
            row["dense_topk_k%d_peak_mib" % k] = peak_mib(lambda: dense_topk(k))
            v, i = m.topk(x, y, k, infer=True)
            dv, di = dense_topk(k)
            row["topk_k%d_indices_equal_to_dense" % k] = round(float((i == di).double().mean()), 6)
            row["topk_k%d_max_abs_value_difference" % k] = float((v - dv).abs().max())
            row["speedup_topk_k%d" % k] = round(row["dense_topk_k%d_ms" % k]["median"] / row["topk_k%d_ms" % k]["median"], 3)
            del v, i, dv, di
        row["rank_of_ms"] = stats(timed(lambda: m.rank_of(x, y, index, infer=True), a.repeats))
        row["dense_rank_ms"] = stats(timed(dense_rank, a.repeats))
        row["rank_of_peak_mib"] = peak_mib(lambda: m.rank_of(x, y, index, infer=True))
        row["dense_rank_peak_mib"] = peak_mib(dense_rank)
        r, dr = m.rank_of(x, y, index, infer=True), dense_rank()
        row["rank_max_abs_difference_from_dense"] = int((r - dr).abs().max())
        row["speedup_rank"] = round(row["dense_rank_ms"]["median"] / row["rank_of_ms"]["median"], 3)
    print(a.only, json.dumps(row), flush=True)
    if a.out:
        res = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                res = json.load(f)
        res[a.only] = row
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
