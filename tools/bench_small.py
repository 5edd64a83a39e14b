#!/usr/bin/env python
"""Latency-regime timings (BASELINE.json configs[2] / configs[4], the reference's real workloads --
sampled sub-graphs).  The datasets are not available offline, so the inputs are sampler-shaped synthetic batches with the
layout facts of the reference pipeline (pyhgt_amd.sampled.synthetic_sampled_batch: type-contiguous ids, `self` runs first,
target-sorted runs, edge_time in [111, 129], min in-degree 1), handed over once through `to_torch`'s wire format
(hgt_plan_build: radix sorts) and once through the device-side hand-off (to_device_graph -> hgt_plan_from_sorted).

--stack B[,B...] [--out FILE]: instead, stacked batches (pyhgt_amd.sampled.stack_device_graphs): for every B, B pieces of the c3
shape (one layer) and of the c5 shape (2-layer GNN) run as ONE block-diagonal graph against the same B pieces run one after the
other, in one process, alternating, medians of 5 windows: us per piece and layer for both, and the time of stack_device_graphs
itself (hgt_stack_sorted + feature gather + plan).  The JSON goes to stdout and, with --out, to FILE.

--trim [--batches 1,16] [--papers 50000] [--only WORKLOAD] [--out FILE]: instead, the seed-trimmed eval forward (GNN.forward(seeds=))
against the untrimmed one read at the seed rows, on the three sampler workloads of tools/bench_sampler.py drawn by the device sampler,
with the README's 4-layer MAG and 2-layer OAG models: alternating windows of ~0.3 s in one process after a warm-up of both, median and
min-max of 5; the trimmed time includes the trim and its plan builds, which are also timed alone.  FILE keeps one JSON object; this
run fills its "eval_forward" (tools/bench_train.py --trim fills the training step and the memory).  --kernels-only: only repeated
trims, for a `rocprofv3 --kernel-trace --stats` run of their launches."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import HGTConv, GNN, GraphPlan  # noqa: E402
from pyhgt_amd.sampled import synthetic_sampled_batch, to_torch_layout, to_device_graph  # noqa: E402


def timeit(fn, iters=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


PRECS = tuple(os.environ.get("HGT_SMALL_PRECS", "bf16x3,f16x3,fp32").split(","))      # e.g. HGT_SMALL_PRECS=f16x3 under rocprofv3


def alternating(fns, iters, warm=10, windows=5):
    """Median us per call of every function, the timed windows of the functions interleaved (window 1 of each, window 2 ...)."""
    for fn in fns:
        for _ in range(warm):
            fn()
    samples = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            samples[i].append(timeit(fn, iters=iters, warm=2))
    return [statistics.median(v) for v in samples]


def stack_bench(dev, Bs, out_path=None, precs=("bf16x3", "f16x3")):
    from pyhgt_amd.sampled import stack_device_graphs
    GraphPlan.CACHE_SIZE = 2 * max(Bs) + 8          # the pieces' plans and the stacks' stay registered
    res = {"stack": list(Bs), "unit": "us per piece and layer (median of 5 alternating windows)"}
    shapes = {"c3": dict(schema="mag", n_seed=128, width=128, depth=6, feat_dim=256, mean_degree=4.0, seed=3, layers=1),
              "c5": dict(schema="oag", n_seed=256, width=128, depth=6, feat_dim=1169, mean_degree=1.2, seed=5, layers=2)}
    for key, c in shapes.items():
        pieces = [to_device_graph(*synthetic_sampled_batch(c["schema"], n_seed=c["n_seed"], width=c["width"], depth=c["depth"],
                                                           feat_dim=c["feat_dim"], mean_degree=c["mean_degree"], seed=c["seed"] + i),
                                  device=dev) for i in range(max(Bs))]
        T, R, L = len(pieces[0][5]), len(pieces[0][6]), c["layers"]
        res[key] = {"N_piece": int(pieces[0][1].numel()), "E_piece": int(pieces[0][4].numel())}
        stacks = {B: stack_device_graphs(pieces[:B]) for B in Bs}
        for B in Bs:
            res[key]["B%d" % B] = {"N": int(stacks[B][1].numel()), "E": int(stacks[B][4].numel()),
                                   "stack_device_graphs_us": timeit(lambda: stack_device_graphs(pieces[:B]), iters=50, warm=5)}
        for prec in precs:
            if key == "c3":
                model = HGTConv(256, 256, T, R, 8, 0.2, True, True, precision=prec).eval().to(dev)
                call = lambda g: model(g[0], g[1], g[3], g[4], g[2], plan=g.plan)
            else:
                model = GNN(1169, 400, T, R, 8, 2, prev_norm=True, last_norm=True, use_RTE=True).eval().to(dev)
                for gc in model.gcs:
                    gc.base_conv.precision = prec
                call = lambda g: model(g[0], g[1], g[2], g[3], g[4])
            with torch.no_grad():
                for B in Bs:
                    S, part = stacks[B], pieces[:B]
                    us_stacked, us_loop = alternating([lambda: call(S), lambda: [call(g) for g in part]], iters=max(10, 100 // B))
                    r = res[key]["B%d" % B]
                    r[prec + "_stacked_us"], r[prec + "_loop_us"] = us_stacked / (B * L), us_loop / (B * L)
                    print("%s x %2d  N=%6d E=%7d %-6s: stacked %7.1f us / piece and layer, one after the other %7.1f, stack_device_graphs "
                          "%.0f us" % (key, B, r["N"], r["E"], prec, r[prec + "_stacked_us"], r[prec + "_loop_us"], r["stack_device_graphs_us"]),
                          flush=True)
        del pieces, stacks
        GraphPlan.clear_cache()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return res


# ------------------------------------------------------------------------------------------------ --trim: the seed-trimmed forward
TRIM_MODELS = {      # the README's models, by the schema of the workload they run on
    "mag": dict(in_dim=129, n_hid=512, H=8, L=4, norm=True),       # the published 4-layer ogbn-mag model
    "oag": dict(in_dim=1169, n_hid=400, H=8, L=2, norm=False),     # the 2-layer OAG model
}


def trim_cases(dev, papers, Bs, only=None):
    """The three sampler workloads of tools/bench_sampler.py (128 seed papers, depth 6), drawn by the device sampler on the synthetic
    resident graphs of examples/train_device_sampler.py: yields (workload, B, graph, seed rows, model spec) for B = 1 (one batch with
    its plan, as sample_subgraph_device hands it over) and B > 1 (one sample_subgraphs_device call, stacked)."""
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from bench_sampler import WORKLOADS
    from pyhgt_amd import sample_subgraph_device, sample_subgraphs_device
    from pyhgt_amd.sampled import stack_device_graphs
    from train_device_sampler import resident_graph
    for name, (schema, depth, width, max_time) in WORKLOADS.items():
        if only and name not in only:
            continue
        m = TRIM_MODELS[schema]
        dgraph, n_nodes = resident_graph(schema, papers, m["in_dim"], dev, seed=1, mean_degree=3.0)
        rng = np.random.default_rng(7)
        for B in Bs:
            inps = [{"paper": np.stack([rng.choice(n_nodes["paper"], 128, replace=False), np.full(128, 2015)], axis=1)} for _ in range(B)]
            keys = [1000 + b for b in range(B)]
            if B == 1:
                g = sample_subgraph_device(dgraph, max_time, depth, width, inps[0], seed=keys[0])
                rows = g.seed_rows("paper")
            else:
                g = stack_device_graphs(sample_subgraphs_device(dgraph, max_time, depth, width, inps, keys, plan=False))
                rows = torch.cat([g.rows(b, "paper", torch.arange(128)) for b in range(B)])
            yield name, B, g, rows, m
            del g
        del dgraph
        GraphPlan.clear_cache()
        torch.cuda.empty_cache()


def trim_shares(t, N, E):
    """rows x layers and edges x layers the trimmed stack still computes, against the untrimmed stack"""
    L = t.n_layers
    return {"nodes": N, "edges": E, "rows_per_stage": list(t.n_rows), "edges_per_layer": list(t.n_edges[1:]),
            "row_share": round(sum(t.n_rows[1:]) / max(1, L * N), 4), "edge_share": round(sum(t.n_edges[1:]) / max(1, L * E), 4)}


def alternating_spread(fns, window_s=0.3, windows=5, warm=5):
    """Per function {median_us, min_us, max_us, iters}: a warm-up of all, then `windows` timed windows of each, interleaved; a window
    repeats the call until it lasts about window_s."""
    for fn in fns:
        for _ in range(warm):
            fn()
    iters = [max(3, int(window_s * 1e6 / max(timeit(fn, iters=3, warm=0), 1.0))) for fn in fns]
    samples = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            samples[i].append(timeit(fn, iters=iters[i], warm=0))
    return [{"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1), "iters": n}
            for v, n in zip(samples, iters)]


def trim_verdict(untrimmed, trimmed):
    """"pays" only where the trimmed median lies below the untrimmed one by more than the two min-max spreads together"""
    spread = (untrimmed["max_us"] - untrimmed["min_us"]) + (trimmed["max_us"] - trimmed["min_us"])
    return {"ratio_trimmed_over_untrimmed": round(trimmed["median_us"] / untrimmed["median_us"], 3),
            "pays": bool(trimmed["median_us"] < untrimmed["median_us"] - spread)}


def merge_out(out_path, key, value):
    """FILE holds one JSON object; this run's part goes under `key`, the other tool's part stays"""
    res = {}
    if out_path and os.path.exists(out_path):
        with open(out_path) as f:
            res = json.load(f)
    res[key] = value
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def trim_bench(dev, Bs, papers, out_path=None, only=None, kernels_only=False):
    """--trim: the eval forward read at the seed rows, untrimmed (plan cached) against trimmed (gnn(..., seeds=rows): the trim, its L
    plan builds and the forward), with the trim alone and the trim with its plans beside them."""
    from pyhgt_amd import trim_to_seeds
    res = {"papers": papers, "seeds": 128, "depth": 6, "unit": "us per call: median, min and max of 5 alternating windows of ~0.3 s", "cases": []}
    for name, B, g, rows, m in trim_cases(dev, papers, Bs, only):
        T, R, L = len(g[5]), len(g[6]), m["L"]
        if kernels_only:                                    # under rocprofv3 --kernel-trace --stats: the trim's own launches
            for _ in range(20):
                trim_to_seeds(g, rows, L)
            continue
        gnn = GNN(m["in_dim"], m["n_hid"], T, R, m["H"], L, prev_norm=m["norm"], last_norm=m["norm"], use_RTE=True).eval().to(dev)

        def plans():
            t = trim_to_seeds(g, rows, L)
            for l in range(1, L + 1):
                t.plan(l, True)
        with torch.no_grad():
            u, t, alone, with_plans = alternating_spread([lambda: gnn(g[0], g[1], g[2], g[3], g[4])[rows],
                                                          lambda: gnn(g[0], g[1], g[2], g[3], g[4], seeds=rows),
                                                          lambda: trim_to_seeds(g, rows, L), plans])
            err = (gnn(g[0], g[1], g[2], g[3], g[4])[rows] - gnn(g[0], g[1], g[2], g[3], g[4], seeds=rows)).abs().max().item()
        case = {"workload": name, "B": B, "layers": L, "n_hid": m["n_hid"], **trim_shares(trim_to_seeds(g, rows, L), g[1].numel(), g[4].numel()),
                "untrimmed": u, "trimmed": t, "trim_alone": alone, "trim_and_plans": with_plans, "max_abs_diff": err, **trim_verdict(u, t)}
        res["cases"].append(case)
        print("%s x %2d  %d layers: untrimmed %.0f us [%.0f, %.0f], trimmed %.0f us [%.0f, %.0f] (trim %.0f, with plans %.0f), row share "
              "%.2f, edge share %.2f, pays: %s" % (name, B, L, u["median_us"], u["min_us"], u["max_us"], t["median_us"], t["min_us"],
                                                   t["max_us"], alone["median_us"], with_plans["median_us"], case["row_share"],
                                                   case["edge_share"], case["pays"]), flush=True)
        del gnn
    if not kernels_only:
        merge_out(out_path, "eval_forward", res)
    return res


def main():
    dev = "cuda:0"
    if "--trim" in sys.argv:
        arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
        trim_bench(dev, [int(v) for v in arg("--batches", "1,16").split(",")], int(arg("--papers", "50000")), arg("--out", None),
                   arg("--only", None), "--kernels-only" in sys.argv)
        return
    if "--stack" in sys.argv:
        Bs = [int(v) for v in sys.argv[sys.argv.index("--stack") + 1].split(",")]
        stack_bench(dev, Bs, sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None)
        return
    res = {}
    # configs[2] surrogate: ogbn-mag sampled sub-graph (sample_depth 6, sample_width 128), T=4 R=9 (incl. self), d=256 H=8
    batch = synthetic_sampled_batch("mag", n_seed=128, width=128, depth=6, feat_dim=256, mean_degree=4.0, seed=3)
    x, nt, tm, ei, et, _, edge_dict = [t.to(dev) if torch.is_tensor(t) else t for t in to_torch_layout(*batch)]
    T, R, d, H = 4, len(edge_dict), 256, 8
    N, E = nt.numel(), et.numel()
    dg = to_device_graph(*batch, device=dev)
    src32, dst32 = dg[3][0].int().contiguous(), dg[3][1].int().contiguous()
    time32 = dg[2].int().contiguous()
    rel_ptr = torch.searchsorted(dg[4], torch.arange(R + 1, device=dev)).int()
    type_off = torch.searchsorted(dg[1], torch.arange(T + 1, device=dev)).int()
    us_build = timeit(lambda: GraphPlan(nt, ei, et, tm, T, R), iters=100, warm=10)
    us_sorted = timeit(lambda: GraphPlan.from_sorted(dg[1], dg[3], dg[4], dg[2], src32, dst32, time32, rel_ptr, type_off, T, R),
                       iters=100, warm=10)
    res["c3"] = {"N": N, "E": E, "plan_build_us": us_build, "plan_from_sorted_us": us_sorted}
    for prec in PRECS:
        layer = HGTConv(d, d, T, R, H, 0.2, True, True, precision=prec).eval().to(dev)
        plan = GraphPlan(nt, ei, et, tm, T, R)
        with torch.no_grad():
            us = timeit(lambda: layer(x, nt, ei, et, tm, plan=plan))
        res["c3"][prec + "_layer_us"] = us
        print("c3 surrogate  N=%d E=%d d=%d %-6s: %.1f us / layer (plan cached), plan build %.1f us (radix) / %.1f us (from sorted), "
              "%.1f M edges/s" % (N, E, d, prec, us, us_build, us_sorted, E / us))
    # configs[4] surrogate: OAG sampled batch, T=5 R=33, batch 256, d=400 H=8, in_dim 1169, 2-layer GNN
    batch = synthetic_sampled_batch("oag", n_seed=256, width=128, depth=6, feat_dim=1169, mean_degree=1.2, seed=5)
    x, nt, tm, ei, et, _, edge_dict = [t.to(dev) if torch.is_tensor(t) else t for t in to_torch_layout(*batch)]
    T, R, d, H, din = 5, len(edge_dict), 400, 8, 1169
    N, E = nt.numel(), et.numel()
    res["c5"] = {"N": N, "E": E}
    for prec in PRECS:
        gnn = GNN(din, d, T, R, H, 2, prev_norm=True, last_norm=True, use_RTE=True).eval().to(dev)
        for gc in gnn.gcs:
            gc.base_conv.precision = prec
        with torch.no_grad():
            us = timeit(lambda: gnn(x, nt, tm, ei, et), iters=100, warm=10)
        res["c5"][prec + "_gnn2_us"] = us
        print("c5 surrogate  N=%d E=%d in=%d d=%d 2-layer GNN %-6s: %.1f us / forward (plan cached)" % (N, E, din, d, prec, us))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
