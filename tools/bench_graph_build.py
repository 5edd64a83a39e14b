#!/usr/bin/env python
"""Building the resident graph from ogbn-mag-shaped raw arrays (pyhgt_amd.synth.synthetic_mag_raw: 1.9 M nodes, 21 M edges, 42 M with
the reverse relations, d = 128), one setting per process:

    python tools/bench_graph_build.py --only a|b|c|d|mean [--scale 1.0] [--repeats 5] [--out profiles/r19_graph_build.json]

  a     DeviceHeteroGraph.from_edge_lists on the device, the edge arrays already resident
  b     the same from host arrays, the upload included
  c     np_edge_lists_to_csr, the numpy definition, on this machine's CPU
  d     the dict build of ogbn-mag/preprocess_ogbn_mag.py:29-42 followed by from_reference_graph, at a TENTH of the size (reported as
        such, not extrapolated)
  mean  neighbour_mean for the author, field and institution features against torch's own chain on the same device: index_add_ of the
        gathered rows, then a division (its row index and counts built outside the clock); bytes = E d 4 gathered + n d 4 written, as a
        fraction of the 7.2 TB/s pure-gather ceiling of profiles/r05_gather_ceiling.txt

A host clock around each call, which ends in a synchronise; after a warm-up call, the median, minimum and maximum over `repeats` calls
(c and d: `--cpu-repeats`, no warm-up).  --out merges the setting into the JSON file, so the five processes fill one file."""
import argparse
import json
import os
import sys
import time
from collections import defaultdict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import DeviceHeteroGraph, neighbour_mean, np_edge_lists_to_csr  # noqa: E402
from pyhgt_amd.synth import synthetic_mag_raw  # noqa: E402

DEV = "cuda:0"
GATHER_CEILING = 7.2e12


def stats(v, digits=2):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits), "n": len(v)}


def timed(fn, repeats, warmup=1, sync=True):
    out = []
    for i in range(warmup + repeats):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        if sync:
            torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
        del res
    return out


class _Stub:
    def __init__(self, types):
        self._types = types
        self.edge_list = defaultdict(lambda: defaultdict(lambda: defaultdict(lambda: defaultdict(dict))))

    def get_types(self):
        return list(self._types)


def dict_build(types, n_nodes, edges, years):
    """lines 29-42 as they stand, then the walk into CSRs"""
    graph = _Stub(types)
    edg = graph.edge_list
    years = years.numpy()
    for key in edges:
        s_type, r_type, t_type = key
        elist = edg[t_type][s_type][r_type]
        rlist = edg[s_type][t_type]["rev_" + r_type]
        for s_id, t_id in edges[key].t().tolist():
            year = None
            if s_type == "paper":
                year = years[s_id]
            elif t_type == "paper":
                year = years[t_id]
            elist[t_id][s_id] = year
            rlist[s_id][t_id] = year
    return DeviceHeteroGraph.from_reference_graph(graph, None, n_nodes=n_nodes)


def torch_mean(rows, src, count, x, n_rows):
    total = torch.zeros(n_rows, x.size(1), device=x.device)
    total.index_add_(0, rows, x[src])
    return total / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", required=True, choices=["a", "b", "c", "d", "mean"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    scale = a.scale * (0.1 if a.only == "d" else 1.0)
    types, n_nodes, edges, x, years = synthetic_mag_raw(scale, a.dim, seed=0)
    row = {"scale_of_ogbn_mag": scale, "nodes": int(sum(n_nodes.values())), "edges": int(sum(v.size(1) for v in edges.values())), "dim": a.dim}
    nt = {"paper": years}
    if a.only in ("a", "b", "mean"):
        row["device_name"] = torch.cuda.get_device_name(0)
    if a.only == "a":
        dev_edges = {k: v.to(DEV) for k, v in edges.items()}
        nt_dev = {"paper": years.to(DEV)}
        row["ms"] = stats(timed(lambda: DeviceHeteroGraph.from_edge_lists(types, n_nodes, dev_edges, node_time=nt_dev, device=DEV), a.repeats))
        g = DeviceHeteroGraph.from_edge_lists(types, n_nodes, dev_edges, node_time=nt_dev, device=DEV)
        row["entries_kept"] = int(sum(c[1].numel() for c in g.csr_dev))
        row["host_reads"] = len(edges)
    elif a.only == "b":
        row["ms"] = stats(timed(lambda: DeviceHeteroGraph.from_edge_lists(types, n_nodes, edges, node_time=nt, device=DEV), a.repeats))
    elif a.only == "c":
        row["ms"] = stats(timed(lambda: np_edge_lists_to_csr(types, n_nodes, edges, None, nt), a.cpu_repeats, warmup=0, sync=False))
        row["cpus"] = os.cpu_count()
    elif a.only == "d":
        row["ms"] = stats(timed(lambda: dict_build(types, n_nodes, edges, years), max(1, a.cpu_repeats - 1), warmup=0, sync=False))
        row["note"] = "a tenth of the size of the other settings; not extrapolated"
    else:
        g = DeviceHeteroGraph.from_edge_lists(types, n_nodes, {k: v.to(DEV) for k, v in edges.items()}, node_time={"paper": years.to(DEV)},
                                              device=DEV)
        xp = x.to(DEV)
        author = torch.empty(n_nodes["author"], a.dim + 1, device=DEV)
        neighbour_mean(g, "author", "paper", xp, out=author[:, :a.dim])
        calls = {"author": ("paper", xp), "field_of_study": ("paper", xp), "institution": ("author", author[:, :a.dim])}
        row["calls"] = {}
        for tt, (st, xs) in calls.items():
            ms = [m for m, (t, s, _) in enumerate(g.triples) if (t, s) == (tt, st)]
            assert len(ms) == 1
            ip, src, _ = g.csr_dev[ms[0]]
            n, E = n_nodes[tt], int(src.numel())
            deg = (ip[1:] - ip[:-1]).long()
            rows, src64, count = torch.repeat_interleave(torch.arange(n, device=DEV), deg), src.long(), deg.clamp(min=1).float()[:, None]
            ours = timed(lambda: neighbour_mean(g, tt, st, xs), a.repeats)
            theirs = timed(lambda: torch_mean(rows, src64, count, xs, n), a.repeats)
            got, want = neighbour_mean(g, tt, st, xs), torch_mean(rows, src64, count, xs, n)
            nbytes = (E + n) * a.dim * 4
            o, t = stats(ours, 3), stats(theirs, 3)
            row["calls"][tt] = {"rows": n, "entries": E, "longest_row": int(deg.max()), "neighbour_mean_ms": o, "torch_index_add_ms": t,
                                "bytes": nbytes, "fraction_of_gather_ceiling": round(nbytes / (o["median"] * 1e-3) / GATHER_CEILING, 3),
                                "faster_than_torch": o["median"] < t["median"],
                                "max_abs_difference_from_torch": float((got - want).abs().max())}
            del rows, src64, count, got, want
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
