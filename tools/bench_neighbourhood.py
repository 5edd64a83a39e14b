#!/usr/bin/env python
"""The exact neighbourhood of a few papers at ogbn-mag size (the graph of tools/bench_whole_graph.py: 1.94 M nodes, 42.2 M CSR
entries, d = 128), one setting per process:

    python tools/bench_neighbourhood.py --only SETTING [--scale 1.0] [--repeats 5] [--out profiles/r22_neighbourhood.json]

  s{S}_l{L}   S in 1, 16, 128, 1024 paper seeds, L in 2, 3 layers (n_hid 256, 8 heads, no RTE: the default of train_ogbn_mag.py):
                neighbourhood      dgraph.neighbourhood({"paper": ids}, L): its rows, edges, host reads and time
                forward            gnn(*nb.inputs, trim=nb) on a fresh neighbourhood, so with its L plan builds
                served             both together
              against two alternatives, measured in the same process with the code paths that were there before:
                seeds_on_view      gnn(*view[:5], seeds=view.rows("paper", ids)) on an already built view, and again with the view's
                                   build (dgraph.whole_graph()) inside the clock
                sampled            one sampled batch of the device sampler (depth 4, width 64) plus its forward: cheap, approximate
              A neighbourhood over --max-rows / --max-edges is recorded as capped, with the level and size the error names.
  x10         the s128_l2 call on the graph and on the graph made ten times larger by nine disconnected copies (the seeds stay in
              the first copy, so the neighbourhood is the same): whether the build time follows the neighbourhood; the ratio is
              written down, whatever it is
  x10_time    the same pair of graphs and the same call with node_time given as host int64 arrays (the form a caller has; a paper's
              year, the graph's last year for every other node): the call that first sees the table objects (validation on the host,
              conversion, upload: work of the graph's size, once per object) and the later calls with the same objects, which use
              the graph's resident copies, each with its x10 ratio

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
from pyhgt_amd import GNN, DeviceHeteroGraph, sample_subgraph_device  # noqa: E402
from pyhgt_amd.synth import synthetic_mag_raw  # noqa: E402

DEV = "cuda:0"
SETTINGS = ["s%d_l%d" % (s, l) for l in (2, 3) for s in (1, 16, 128, 1024)] + ["x10", "x10_time"]


def stats(v, digits=3):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits), "n": len(v)}


def timed(fn, repeats, warmup=1, before=None):
    out = []
    for i in range(warmup + repeats):
        arg = before() if before else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(arg) if before else fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
        del res, arg
    return out


def graph(scale, dim, copies=1):
    types, n_nodes, edges, x, years = synthetic_mag_raw(scale, dim, seed=0)
    gen = torch.Generator().manual_seed(1)
    feats = {t: (x if t == "paper" else torch.randn(n_nodes[t], dim, generator=gen)).to(DEV) for t in types}
    edges = {k: v.to(DEV) for k, v in edges.items()}
    years = years.to(DEV)
    if copies > 1:                                           # disconnected copies: every id of copy c shifted by c * n_type
        shift = lambda k, c: torch.tensor([[c * n_nodes[k[0]]], [c * n_nodes[k[2]]]], device=DEV)
        edges = {k: torch.cat([v + shift(k, c) for c in range(copies)], dim=1) for k, v in edges.items()}
        feats = {t: f.repeat(copies, 1) for t, f in feats.items()}
        years = years.repeat(copies)
        n_nodes = {t: n * copies for t, n in n_nodes.items()}
    g = DeviceHeteroGraph.from_edge_lists(types, n_nodes, edges, node_time={"paper": years}, features=feats, device=DEV)
    return g, n_nodes, years


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", required=True, choices=SETTINGS)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--hid", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=1500000)
    ap.add_argument("--max-edges", type=int, default=30000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g, n_nodes, years = graph(a.scale, a.dim)
    P = n_nodes["paper"]
    T, R = len(g.types), len(g.edge_dict)
    row = {"scale_of_ogbn_mag": a.scale, "nodes": int(sum(g.n_nodes)), "csr_entries": int(sum(c[1].numel() for c in g.csr_dev)), "dim": a.dim,
           "device_name": torch.cuda.get_device_name(0)}
    if a.only == "x10_time":
        ids = torch.from_numpy(np.random.default_rng(128).integers(0, P, 128)).to(DEV)
        last = int(years.max())

        def tables(gr, yrs):
            return {t: (yrs.cpu().numpy().astype(np.int64) if t == "paper" else np.full(n, last, np.int64)) for t, n in zip(gr.types, gr.n_nodes)}

        def measure(gr, yrs, tag):
            kept = tables(gr, yrs)
            nb = gr.neighbourhood({"paper": ids}, 2, node_time=kept)
            row["rows" + tag], row["edges" + tag], row["host_reads" + tag] = nb.n_rows[0], nb.n_edges[1], nb.host_reads
            row["no_node_time" + tag + "_ms"] = stats(timed(lambda: gr.neighbourhood({"paper": ids}, 2), a.repeats))
            row["tables_seen_before" + tag + "_ms"] = stats(timed(lambda: gr.neighbourhood({"paper": ids}, 2, node_time=kept), a.repeats))
            row["new_table_objects" + tag + "_ms"] = stats(timed(lambda tb: gr.neighbourhood({"paper": ids}, 2, node_time=tb), a.repeats,
                                                                 before=lambda: tables(gr, yrs)))
            gr.forget_neighbourhood_tables()
        row.update(seeds=128, n_layers=2, node_time="host int64 arrays, one per type")
        measure(g, years, "")
        del g
        torch.cuda.empty_cache()
        g10, _, years10 = graph(a.scale, a.dim, copies=10)
        row["nodes_x10"], row["csr_entries_x10"] = int(sum(g10.n_nodes)), int(sum(c[1].numel() for c in g10.csr_dev))
        measure(g10, years10, "_x10")
        for k in ("no_node_time", "tables_seen_before", "new_table_objects"):
            row["ratio_x10_over_x1_" + k] = round(row[k + "_x10_ms"]["median"] / row[k + "_ms"]["median"], 3)
    elif a.only == "x10":
        ids = torch.from_numpy(np.random.default_rng(128).integers(0, P, 128)).to(DEV)
        call = lambda gr: gr.neighbourhood({"paper": ids}, 2)
        nb = call(g)
        row.update(seeds=128, n_layers=2, rows=nb.n_rows[0], edges=nb.n_edges[1])
        row["neighbourhood_ms"] = stats(timed(lambda: call(g), a.repeats))
        del g
        torch.cuda.empty_cache()
        g10, _, _ = graph(a.scale, a.dim, copies=10)
        nb10 = call(g10)
        assert nb10.n_rows == nb.n_rows and nb10.n_edges == nb.n_edges, "the copies are not disconnected"
        row["nodes_x10"], row["csr_entries_x10"] = int(sum(g10.n_nodes)), int(sum(c[1].numel() for c in g10.csr_dev))
        row["first_call_x10_ms"] = "not timed (it allocates and clears the marks)"
        row["neighbourhood_x10_ms"] = stats(timed(lambda: call(g10), a.repeats))
        row["ratio_x10_over_x1"] = round(row["neighbourhood_x10_ms"]["median"] / row["neighbourhood_ms"]["median"], 3)
    else:
        S, L = (int(v[1:]) for v in a.only.split("_"))
        ids = torch.from_numpy(np.random.default_rng(S).integers(0, P, S)).to(DEV)
        torch.manual_seed(0)
        gnn = GNN(a.dim, a.hid, T, R, 8, L, 0.2, "hgt", True, True, False).to(DEV).eval()
        row.update(seeds=S, n_layers=L, n_hid=a.hid, max_rows=a.max_rows, max_edges=a.max_edges)
        build = lambda: g.neighbourhood({"paper": ids}, L, max_rows=a.max_rows, max_edges=a.max_edges)
        with torch.no_grad():
            try:
                nb = build()
                row.update(rows=nb.n_rows[0], edges=nb.n_edges[1], rows_per_layer=list(nb.n_rows), host_reads=nb.host_reads)
                row["neighbourhood_ms"] = stats(timed(build, a.repeats))
                row["forward_with_plans_ms"] = stats(timed(lambda n: gnn(*n.inputs, trim=n), a.repeats, before=build))
                row["served_ms"] = stats(timed(lambda: (lambda n: gnn(*n.inputs, trim=n))(build()), a.repeats))
                out_nb = gnn(*nb.inputs, trim=nb)
            except OverflowError as e:
                nb, out_nb = None, None
                row["capped"] = str(e)
                row["capped_call_ms"] = stats(timed(lambda: _capped(build), a.repeats))
            # ---- the alternatives, with the code paths that were there before
            view = g.whole_graph()
            seeds = view.rows("paper", ids)
            row["view_edges"] = int(view[3].size(1))
            row["seeds_on_built_view_ms"] = stats(timed(lambda: gnn(*view[:5], seeds=seeds), a.repeats))
            if out_nb is not None:
                row["max_abs_difference_from_seeds_on_view"] = float((gnn(*view[:5], seeds=seeds) - out_nb).abs().max())
            del view
            torch.cuda.empty_cache()

            def with_view():
                v = g.whole_graph()
                return gnn(*v[:5], seeds=v.rows("paper", ids))
            row["seeds_with_view_build_ms"] = stats(timed(with_view, a.repeats))
            inp = {"paper": np.stack([ids.cpu().numpy(), years[ids].cpu().numpy()], axis=1)[np.unique(ids.cpu().numpy(), return_index=True)[1]]}

            def sampled():
                sub = sample_subgraph_device(g, None, 4, 64, inp, seed=1)
                return gnn(*sub[:5])[sub.seed_rows("paper")]
            row["sampled_batch_and_forward_ms"] = stats(timed(sampled, a.repeats))
            sub = sample_subgraph_device(g, None, 4, 64, inp, seed=1)
            row["sampled_rows"], row["sampled_edges"] = int(sub[1].numel()), int(sub[3].size(1))
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


def _capped(build):
    try:
        build()
    except OverflowError:
        pass


if __name__ == "__main__":
    main()
