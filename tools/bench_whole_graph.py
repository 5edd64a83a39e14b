#!/usr/bin/env python
"""The whole-graph view at ogbn-mag size (pyhgt_amd.synth.synthetic_mag_raw, the arrays of tools/bench_graph_build.py: 1.9 M nodes,
42 M entries with the reverse relations), one setting per process:

    python tools/bench_whole_graph.py --only SETTING [--scale 1.0] [--repeats 5] [--out profiles/r21_whole_graph.json]

  build          dgraph.whole_graph(plan=False), unfiltered: one launch, no host read
  build_filtered the same with max_time = 2016: count, scan, fill and the one host read
  build_plan     the unfiltered view with its plan (hgt_plan_from_sorted)
  numpy          np_whole_graph on this machine's CPU plus the upload of its int32 arrays and feature matrix: what a caller without
                 the device build would do
  forward2 / forward4   the eval forward of a 2- / 4-layer GNN (n_hid 256, 8 heads, no RTE: the default of train_ogbn_mag.py) over
                 the whole graph: time and peak memory
  eval           the exact evaluation of all test papers (one whole forward of the 2-layer model + Classifier.predict) against the
                 voted evaluation of the parent commit's path (sample_subgraphs_device x vr_num, stack, forward, vote per chunk of 128
                 test papers) over the first --chunks chunks; reported per chunk and not extrapolated

A host clock around each call, which ends in a synchronise; after a warm-up call, the median, minimum and maximum over `repeats` calls.
--out merges the setting into the JSON file, so the processes fill one file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import GNN, Classifier, DeviceHeteroGraph, VoteTable, np_whole_graph, sample_subgraphs_device  # noqa: E402
from pyhgt_amd.sampled import stack_device_graphs  # noqa: E402
from pyhgt_amd.synth import synthetic_mag_raw  # noqa: E402

DEV = "cuda:0"
SETTINGS = ["build", "build_filtered", "build_plan", "numpy", "forward2", "forward4", "eval"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", required=True, choices=SETTINGS)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--hid", type=int, default=256)
    ap.add_argument("--classes", type=int, default=349)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--vr-num", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    types, n_nodes, edges, x, years = synthetic_mag_raw(a.scale, a.dim, seed=0)
    gen = torch.Generator().manual_seed(1)
    feats = {t: (x if t == "paper" else torch.randn(n_nodes[t], a.dim, generator=gen)) for t in types}
    g = DeviceHeteroGraph.from_edge_lists(types, n_nodes, {k: v.to(DEV) for k, v in edges.items()}, node_time={"paper": years.to(DEV)},
                                          features={t: f.to(DEV) for t, f in feats.items()}, device=DEV)
    T, R = len(g.types), len(g.edge_dict)
    entries = int(sum(c[1].numel() for c in g.csr_dev))
    row = {"scale_of_ogbn_mag": a.scale, "nodes": int(sum(g.n_nodes)), "csr_entries": entries, "dim": a.dim,
           "device_name": torch.cuda.get_device_name(0)}
    if a.only in ("build", "build_filtered", "build_plan"):
        kw = dict(max_time=2016) if a.only == "build_filtered" else {}
        plan = a.only == "build_plan"
        row["ms"] = stats(timed(lambda: g.whole_graph(plan=plan, **kw), a.repeats))
        v = g.whole_graph(plan=plan, **kw)
        row["edges"] = int(v[3].size(1))
        row["host_reads"] = 1 if kw else 0
        # streamed per entry: src (+ time under max_time) and a share of indptr in; src32, dst32, edge_index (2 x int64), edge_type out
        row["bytes_out_per_edge"] = 4 + 4 + 16 + 8
        row["note"] = "includes the concatenation of the feature matrices (%d x %d float32)" % (row["nodes"], a.dim)
        feat_ms = stats(timed(lambda: torch.cat([f for f in g.features]), a.repeats))
        row["feature_concatenation_ms"] = feat_ms
    elif a.only == "numpy":
        g.csr                                                        # (the download of the CSRs is outside the clock,
        g.features_host = [feats[t].numpy() for t in g.types]       #  and the features start on the host)

        def host_path():
            arr = np_whole_graph(g)
            up = [torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in arr.sorted if v is not None]
            return up, torch.from_numpy(arr.node_feature).to(DEV)
        row["ms"] = stats(timed(host_path, max(1, a.repeats // 2), warmup=0))
        row["cpus"] = os.cpu_count()
    else:
        L = 4 if a.only == "forward4" else 2
        torch.manual_seed(0)
        gnn = GNN(a.dim, a.hid, T, R, 8, L, 0.2, "hgt", True, True, False).to(DEV).eval()
        view = g.whole_graph()
        row.update(edges=int(view[3].size(1)), n_hid=a.hid, n_layers=L)
        if a.only != "eval":
            with torch.no_grad():
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                row["ms"] = stats(timed(lambda: gnn(*view[:5]), a.repeats))
                row["peak_memory_gib_above_graph_and_view"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 2)
                row["graph_and_view_gib"] = round(base / 2 ** 30, 2)
        else:
            head = Classifier(a.hid, a.classes).to(DEV).eval()
            P = n_nodes["paper"]
            y = torch.randint(0, a.classes, (P,), generator=gen).to(DEV)
            split_host = torch.where(years <= 2017, 0, torch.where(years == 2018, 1, 2)).to(torch.int32)
            split = split_host.to(DEV)
            test_paper = np.flatnonzero(split_host.numpy() == 2)
            ids = torch.arange(P, device=DEV)
            paper = view.type_rows("paper")

            def exact():
                return head.predict(gnn(*view[:5])[paper], ids=ids, labels=y, split=split, n_splits=3)[1].tolist()

            years_np = years.numpy()
            table = VoteTable(P, a.classes, nodes=test_paper, device=DEV)

            def voted_chunk(lo):
                chunk = test_paper[lo:lo + 128]
                inp = {"paper": np.stack([chunk, years_np[chunk]], axis=1)}
                pieces = sample_subgraphs_device(g, None, 4, 64, [inp] * a.vr_num, [1000 * lo + b for b in range(a.vr_num)], plan=False)
                s = stack_device_graphs(pieces)
                pid = torch.cat([p.indxs["paper"] for p in pieces])
                rep = gnn(s[0], s[1], s[2], s[3], s[4])[s[5]["paper"][0]:s[5]["paper"][0] + pid.numel()]
                head.vote(rep, table, pid, piece_sizes=[p.indxs["paper"].numel() for p in pieces])

            with torch.no_grad():
                row["exact_all_papers_ms"] = stats(timed(exact, a.repeats))
                voted_chunk(0)
                per_chunk = []
                for c in range(1, a.chunks + 1):
                    per_chunk += timed(lambda: voted_chunk(128 * c), 1, warmup=0)
                row["voted_ms_per_chunk_of_128"] = stats(per_chunk)
            row["test_papers"] = int(test_paper.size)
            row["chunks_of_128_for_all_test_papers"] = int((test_paper.size + 127) // 128)
            row["vr_num"] = a.vr_num
            row["note"] = "voted: %d chunks measured, not extrapolated; exact covers all %d papers of every split" % (a.chunks, P)
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
