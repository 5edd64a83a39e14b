#!/usr/bin/env python
"""Time per sampled batch: sample_subgraph_device against its numpy sibling sample_subgraph_host and, for scale, to_device_graph on the
host sibling's output, on MAG- and OAG-shaped synthetic resident graphs (the schemas of pyhgt_amd/sampled.py) at the reference's batch
shapes: 128 seed papers, depth 6, width 128 (OAG/train_paper_field.py) and width 520 (ogbn-mag/train_ogbn_mag.py:44-55).

    python tools/bench_sampler.py [--papers 200000] [--reps 10] [--host-reps 2] [--out profiles/r11_device_sampler.json]
    python tools/bench_sampler.py --task [--out profiles/r12_task_batches.json]
    python tools/bench_sampler.py --batch 1,4,16 [--reps 10] [--out profiles/r13_batched_sampler.json]

--task times a task batch instead (the OAG workload only): the call with the label edges at the 128 seed papers masked out
(mask=seed_edge_mask(...), the same launches as the plain call) against the plain call, alternating in one process, medians of 8 each;
and LabelSpace.distribution / LabelSpace.index for the 128 seeds (one launch each).

--batch B[,B...] times the batched call instead: for every B one sample_subgraphs_device call of B batches against B
sample_subgraph_device calls in a loop (the same seeds and Philox seeds, alternating in one process, medians of --reps), the time per
batch of both, and the launches of both counted from the calls the host loops make.

Device time is wall-clock per call with a synchronisation after each (the call synchronises once by itself, for the sizes of the
result); launches per batch are counted from the calls the host loop makes (every C entry point is a fixed number of launches).  One
JSON line per workload on stdout, all of them in --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from pyhgt_amd import LabelSpace, sample_subgraph_device, sample_subgraph_host, sample_subgraphs_device, seed_edge_mask  # noqa: E402
from pyhgt_amd.sampled import SchemaGraph, to_device_graph  # noqa: E402
from train_device_sampler import resident_graph  # noqa: E402

WORKLOADS = {"oag_d6_w128": ("oag", 6, 128, 2015), "mag_d6_w520": ("mag", 6, 520, None), "mag_d6_w128": ("mag", 6, 128, None)}
# launches per C entry point (csrc/hgt_sampler.hip): seed 1, add_budget memset + 2, select 2, induce_count memset + 3, induce_fill 3, reset 2
LAUNCHES = dict(seed=1, add_budget=3, select=2, induce=7, reset=2)


def launches_per_batch(dgraph, depth, n_seed_types=1):
    T = len(dgraph.types)
    live = sum(1 for t in range(T) if any(st == t for _, st, _ in dgraph.tri_types))
    feature_gathers = T
    return (n_seed_types * (LAUNCHES["seed"] + LAUNCHES["add_budget"]) + depth * live * (LAUNCHES["select"] + LAUNCHES["add_budget"])
            + LAUNCHES["induce"] + LAUNCHES["reset"] + feature_gathers)


def launches_per_batched_call(dgraph, depth, n_seed_types=1):
    """the launches of one sample_subgraphs_device call, whatever B is: those of a single batch with one more in the fill pass (the
    prefix sums over the replicas) and ONE feature gather for all types and replicas"""
    T = len(dgraph.types)
    live = sum(1 for t in range(T) if any(st == t for _, st, _ in dgraph.tri_types))
    return (n_seed_types * (LAUNCHES["seed"] + LAUNCHES["add_budget"]) + depth * live * (LAUNCHES["select"] + LAUNCHES["add_budget"])
            + LAUNCHES["induce"] + 1 + LAUNCHES["reset"] + 1)


def batch_lines(a, dev):
    """per workload and B: one batched call against B single calls in a loop"""
    sizes = [int(v) for v in a.batch.split(",")]
    lines = []
    for name, (schema, depth, width, max_time) in WORKLOADS.items():
        dgraph, n_nodes = resident_graph(schema, a.papers, a.feat_dim, dev, seed=1, mean_degree=a.mean_degree)
        rng = np.random.default_rng(7)
        draw = lambda: {"paper": np.stack([rng.choice(n_nodes["paper"], 128, replace=False), np.full(128, 2015)], axis=1)}
        per_b = []
        for B in sizes:
            rounds = [([draw() for _ in range(B)], [1000 * r + b for b in range(B)]) for r in range(a.reps + 1)]
            loop = lambda inps, keys: [sample_subgraph_device(dgraph, max_time, depth, width, i, seed=k, plan=False) for i, k in zip(inps, keys)]
            one = lambda inps, keys: sample_subgraphs_device(dgraph, max_time, depth, width, inps, keys, plan=False)
            loop(*rounds[0]), one(*rounds[0])                # warm-up: allocations of both states, first launches
            torch.cuda.synchronize()
            t_loop, t_one = [], []
            for r in range(1, a.reps + 1):
                for fn, t in ((loop, t_loop), (one, t_one)) if r % 2 else ((one, t_one), (loop, t_loop)):
                    dt, out = _timed(lambda: fn(*rounds[r]))
                    t.append(dt)
            ms = lambda v: float(np.median(v) * 1e3)
            per_b.append(dict(batch=B, batched_call_ms=ms(t_one), batched_ms_per_batch=ms(t_one) / B, batched_call_ms_min=float(np.min(t_one) * 1e3),
                              loop_ms=ms(t_loop), loop_ms_per_batch=ms(t_loop) / B, launches_batched_call=launches_per_batched_call(dgraph, depth),
                              launches_loop=B * launches_per_batch(dgraph, depth), nodes_last_call=int(sum(g[1].numel() for g in out))))
        line = dict(workload=name, schema=schema, papers=a.papers, seeds=128, depth=depth, width=width, reps=a.reps, per_batch_size=per_b)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del dgraph
    return lines


def hand_over(res, dgraph):
    """the host sibling's result as (feature, time, edge_list, graph) for to_device_graph"""
    types = dgraph.get_types()
    src, dst, _, rel_ptr, off = res.sorted
    feat = res[0].numpy()
    feature = {t: feat[off[i]:off[i + 1]] for i, t in enumerate(types)}
    edge_list = {}
    for i, t in enumerate(types):
        n = int(off[i + 1] - off[i])
        if n:
            edge_list.setdefault(t, {}).setdefault(t, {})["self"] = np.stack([np.arange(n), np.arange(n)], axis=1)
    tid = {t: i for i, t in enumerate(types)}
    for tt, st, rel in dgraph.triples:
        r = dgraph.edge_dict[rel]
        e = slice(rel_ptr[r], rel_ptr[r + 1])
        if rel_ptr[r + 1] > rel_ptr[r]:
            edge_list.setdefault(tt, {}).setdefault(st, {})[rel] = np.stack([dst[e] - off[tid[tt]], src[e] - off[tid[st]]], axis=1)
    return feature, res.times, edge_list, SchemaGraph(types, dgraph.get_meta_graph())


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def task_line(a, dev):
    """masked against plain call, alternating in the same windows, and the two label calls, on the OAG workload"""
    name = "oag_d6_w128"
    schema, depth, width, max_time = WORKLOADS[name]
    dgraph, n_nodes = resident_graph(schema, a.papers, a.feat_dim, dev, seed=1, mean_degree=a.mean_degree)
    relations = ["PF_in_L2", "rev_PF_in_L2", "PV_Journal", "rev_PV_Journal"]
    mask = seed_edge_mask(dgraph, relations, "paper", 128)
    fields = LabelSpace(dgraph, ("paper", "field", "PF_in_L2"), np.arange(n_nodes["field"]))
    venues = LabelSpace(dgraph, ("paper", "venue", "PV_Journal"), np.arange(n_nodes["venue"]))
    rng = np.random.default_rng(7)
    reps = 8
    inps = [{"paper": np.stack([rng.choice(n_nodes["paper"], 128, replace=False), np.full(128, 2015)], axis=1)} for _ in range(reps + 2)]
    for i in range(2):                                       # warm-up of both forms and of the label kernel
        g = sample_subgraph_device(dgraph, max_time, depth, width, inps[i], seed=i, mask=mask if i else None)
        fields.distribution(g.indxs["paper"][:128]), venues.index(g.indxs["paper"][:128])
    torch.cuda.synchronize()
    t = dict(plain=[], masked=[], distribution=[], index=[])
    removed = []
    for i in range(reps):
        order = [("plain", None), ("masked", mask)] if i % 2 == 0 else [("masked", mask), ("plain", None)]
        got = {}
        for key, m in order:
            dt, got[key] = _timed(lambda: sample_subgraph_device(dgraph, max_time, depth, width, inps[2 + i], seed=100 + i, mask=m))
            t[key].append(dt)
        removed.append(int(got["plain"][4].numel() - got["masked"][4].numel()))
        seeds = got["masked"].indxs["paper"][:128]
        t["distribution"].append(_timed(lambda: fields.distribution(seeds))[0])
        t["index"].append(_timed(lambda: venues.index(seeds))[0])
    ms = lambda v: float(np.median(v) * 1e3)
    spread = lambda v: [float(np.min(v) * 1e3), float(np.max(v) * 1e3)]
    return dict(workload=name + "_task", papers=a.papers, seeds=128, depth=depth, width=width, reps=reps, masked_relations=relations,
                batch_edges=int(got["plain"][4].numel()), edges_masked_median=int(np.median(removed)),
                launches_per_batch=launches_per_batch(dgraph, depth), plain_ms=ms(t["plain"]), plain_ms_min_max=spread(t["plain"]),
                masked_ms=ms(t["masked"]), masked_ms_min_max=spread(t["masked"]), label_classes=[fields.n_cols, venues.n_cols],
                label_distribution_ms=ms(t["distribution"]), label_index_ms=ms(t["index"]), label_launches=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--papers", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--feat-dim", type=int, default=128)
    ap.add_argument("--mean-degree", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--task", action="store_true")
    ap.add_argument("--batch", default=None, help="batch sizes of the batched call, e.g. 1,4,16")
    a = ap.parse_args()
    dev, lines = "cuda:0", []
    if a.task:
        lines.append(task_line(a, dev))
        print(json.dumps(lines[0]), flush=True)
    if a.batch:
        lines += batch_lines(a, dev)
    for name, (schema, depth, width, max_time) in ({} if a.task or a.batch else WORKLOADS).items():
        dgraph, n_nodes = resident_graph(schema, a.papers, a.feat_dim, dev, seed=1, mean_degree=a.mean_degree)
        rng = np.random.default_rng(7)
        inps = [{"paper": np.stack([rng.choice(n_nodes["paper"], 128, replace=False), np.full(128, 2015)], axis=1)} for _ in range(a.reps + 2)]
        for i in range(2):                                   # warm-up: allocations of the state, first launches
            g = sample_subgraph_device(dgraph, max_time, depth, width, inps[i], seed=i)
        torch.cuda.synchronize()
        t_dev = []
        for i in range(a.reps):
            t0 = time.perf_counter()
            g = sample_subgraph_device(dgraph, max_time, depth, width, inps[2 + i], seed=100 + i)
            torch.cuda.synchronize()
            t_dev.append(time.perf_counter() - t0)
        t_host, t_hand = [], []
        for i in range(a.host_reps):
            t0 = time.perf_counter()
            h = sample_subgraph_host(dgraph, max_time, depth, width, inps[2 + i], seed=100 + i)
            t_host.append(time.perf_counter() - t0)
            args = hand_over(h, dgraph)
            t0 = time.perf_counter()
            to_device_graph(*args, device=dev)
            torch.cuda.synchronize()
            t_hand.append(time.perf_counter() - t0)
        line = dict(workload=name, schema=schema, papers=a.papers, nodes_total=int(sum(n_nodes.values())),
                    edges_total=int(sum(c[1].size for c in dgraph.csr)), max_degree=int(max(np.diff(c[0]).max() for c in dgraph.csr)),
                    seeds=128, depth=depth, width=width, batch_nodes=int(g[1].numel()), batch_edges=int(g[4].numel()),
                    launches_per_batch=launches_per_batch(dgraph, depth), device_ms_per_batch=float(np.median(t_dev) * 1e3),
                    device_ms_min=float(np.min(t_dev) * 1e3), host_sibling_ms_per_batch=float(np.median(t_host) * 1e3),
                    to_device_graph_ms=float(np.median(t_hand) * 1e3), host_batch_nodes=int(h[1].numel()))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del dgraph
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
