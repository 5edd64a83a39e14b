#!/usr/bin/env python
"""Training-step timing of one HGTConv at BASELINE.json configs[1]: forward + backward through
pyhgt_amd/autograd.py against the inference forward, plan (and transposed plan) cached.  Sizes from the environment: HGT_TRAIN_N,
HGT_TRAIN_E (nodes, edges), HGT_TRAIN_D, HGT_TRAIN_H (width, heads); HGT_TRAIN_NO_SMALL=1 skips the sampled-batch part.
--deterministic (or HGT_TRAIN_DETERMINISTIC=1) times the bit-reproducible mode (deterministic=True on every module).
--emulate-world W [--out FILE]: instead, the training step of ONE rank of a W-rank destination partition on one GPU, the recipe of
bench.py --emulate-world (exact receive side, mirrored send side, the all-to-alls replaced by device copies of as many bytes):
forward, backward and, inside the backward, the return of the halo gradients, of one layer; the JSON line is appended to FILE.
--recompute [--out FILE]: instead, the memory-lean mode (recompute=True) against the default mode in ONE process: the layer step of
the sizes above in both modes, alternating (5 warm-ups, median of 20, events on the compute stream), hgt_dropout_apply against
hgt_mul_inplace at n = 2^28, and torch.cuda.max_memory_allocated() of a four-layer step in each mode; FILE is written as JSON.
--stack B[,B...] [--out FILE]: instead, the sampled-size training step (c3 layer, c5 2-layer GNN; forward + backward, dropout on) on
B stacked batches (pyhgt_amd.sampled.stack_device_graphs) against the same B batches stepped one after the other, in one process,
alternating, medians of 5 windows: ms per piece.
--optimizer {none,torch,device} (default none: the numbers above do not move): the sampled-batch steps end in an optimizer step over
the module's parameters -- torch: clip_grad_norm_(0.5) + torch.optim.AdamW; device: pyhgt_amd.AdamW(max_norm=0.5) -- so that three runs
give the share of a step the optimizer is (tools/bench_optimizer.py times the optimizer step alone).
--trim [--batches 1,16] [--papers 50000] [--only WORKLOAD] [--out FILE]: instead, the training step of the seed-trimmed forward
(GNN.forward(seeds=), the trim and its plan builds inside the step) against the untrimmed step read at the seed rows, on the sampler
workloads and models of tools/bench_small.py --trim, alternating windows of ~0.3 s, median and min-max of 5; and
torch.cuda.max_memory_allocated() / the memory kept after the forward of a 4-layer step in both forms.  FILE keeps one JSON object;
this run fills its "training_step"."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import HGTConv, GraphPlan  # noqa: E402
from pyhgt_amd.synth import synthetic_typed_graph  # noqa: E402


def training_step_bytes(N, E, d, H):
    """Algorithmic HBM bytes of one training step of HGTConv (4-argument form, LayerNorm on) in the same minimal-traffic convention
    as the forward's SURVEY 8(d) model: every kernel reads its inputs and writes its outputs once, every edge gathers one 4d-byte
    row per gather pass (no cache-reuse credit), ids cost 12 B per edge and pass, weights are ignored.  Kernel by kernel, in the
    order the steps of pyhgt_amd/autograd.py enqueue them: project, attention, aggregate, update_hgt; then update_hgt_bwd,
    attention_bwd, qkv_bwd, relation_bwd, project_bwd."""
    Nd, EH, Eg = N * 4 * d, E * H * 4, E * (4 * d + 12)          # one fp32 feature array / one per-edge-per-head array / one gather pass
    fwd = {"project_qkv": 4 * Nd, "edge_logits": Eg + Nd + EH, "edge_softmax": 2 * EH, "edge_aggregate": Eg + EH + Nd,
           "a_linear": 2 * Nd, "node_update": 3 * Nd}
    bwd = {"node_update_bwd": 5 * Nd,                              # read grad_out, trans, x; write d_trans, dx_skip
           "gelu(agg)": 2 * Nd, "wgrad_a": 2 * Nd, "d_gelu = d_trans W_a": 2 * Nd, "gelu_bwd": 3 * Nd,
           "d_att (logits kernel on dagg, V, M^T)": Eg + Nd + EH, "head_dot rho": 2 * Nd, "softmax_bwd": 3 * EH,
           "spmm dQ": Eg + EH + Nd, "re-sort ds, att to the transposed plan": 8 * EH, "spmm dK": Eg + EH + Nd, "spmm dV": Eg + EH + Nd,
           "outer d relation_msg": Eg + EH + Nd, "outer d relation_att": Eg + EH + Nd,
           "wgrad_qkv": 4 * Nd, "dx = dqkv W_qkv": 4 * Nd, "dx += dx_skip": 3 * Nd}
    return fwd, bwd


def minimal_backward_bytes(N, E, d, H):
    """A MINIMAL-traffic model of the backward (round-5 review: the figure above counts the kernels as built -- seven E x d gather passes).
    What the arithmetic needs at least: ONE walk in target order that gathers K_j and V_j per edge (d att = <d agg' M^T, v>, the softmax
    backward in registers, dQ_i summed in place -- Q_i and d agg_i are read once per target -- and d relation_att / d relation_msg as
    outer products of rows already in flight), which leaves d s [E, H] behind, and ONE walk in source order that gathers the target-side
    rows q~_i and d agg'_i per edge to sum dK_j and dV_j: four gather passes, two per-edge-per-head arrays written and read once, every
    node-level array read or written once per GEMM that needs it."""
    Nd, EH, Eg = N * 4 * d, E * H * 4, E * (4 * d + 12)
    return {"node_update_bwd + a_linear bwd (read grad_out, trans, x, agg; write d agg, dx_skip; W_a gradient reads agg, d_trans)": 9 * Nd,
            "target-order walk (gather K, V; read Q, d agg; write dQ, d s)": 2 * Eg + 3 * Nd + 2 * EH,
            "source-order walk (gather q~, d agg'; read d s, att; write dK, dV)": 2 * Eg + 2 * Nd + 2 * EH,
            "Q|K|V weight gradients + dx (read x, dQ|dK|dV; write dx)": 8 * Nd}


DETERMINISTIC = "--deterministic" in sys.argv or os.environ.get("HGT_TRAIN_DETERMINISTIC", "0") not in ("", "0")
OPTIMIZER = sys.argv[sys.argv.index("--optimizer") + 1] if "--optimizer" in sys.argv else "none"
assert OPTIMIZER in ("none", "torch", "device"), "--optimizer {none,torch,device}"


def optimizer_step(params):
    """the call that ends a step under --optimizer (None: the gradients are dropped, as before)"""
    if OPTIMIZER == "none":
        return None
    if OPTIMIZER == "torch":
        opt = torch.optim.AdamW(params, lr=1e-3)
        return lambda: (torch.nn.utils.clip_grad_norm_(params, 0.5), opt.step())
    import pyhgt_amd
    return pyhgt_amd.AdamW(params, lr=1e-3, max_norm=0.5).step


def sampled_batches(dev):
    """Training step (forward + backward, dropout on) at the sizes the reference's scripts actually step on (round-5 review, task 8):
    the c3 surrogate (one layer, d = 256) and the c5 / published ogbn-mag surrogates (whole GNN), wall-clock us per step."""
    from pyhgt_amd import GNN
    from pyhgt_amd.sampled import synthetic_sampled_batch, to_torch_layout
    res = {}

    def step_us(fn, params, module, iters=30):
        opt_step = optimizer_step(list(module.parameters()))
        for it in range(5 + iters):
            if it == 5:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            out = fn()
            out.backward(torch.ones_like(out))
            if opt_step is not None:
                opt_step()
            for p_ in params:
                p_.grad = None
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    batch = synthetic_sampled_batch("mag", n_seed=128, width=128, depth=6, feat_dim=256, mean_degree=4.0, seed=3)
    x, nt, tm, ei, et, _, ed = [t.to(dev) if torch.is_tensor(t) else t for t in to_torch_layout(*batch)]
    layer = HGTConv(256, 256, 4, len(ed), 8, 0.2, True, True, deterministic=DETERMINISTIC).to(dev).train()
    plan = GraphPlan(nt, ei, et, tm, 4, len(ed))
    xg = x.clone().requires_grad_(True)
    res["c3_layer"] = {"N": int(nt.numel()), "E": int(et.numel()), "d": 256,
                       "fwd_bwd_us": step_us(lambda: layer(xg, nt, ei, et, tm, plan=plan), list(layer.parameters()) + [xg], module=layer)}
    for key, c in (("c5_gnn2", dict(schema="oag", n_seed=256, width=128, depth=6, feat_dim=1169, mean_degree=1.2, seed=5, in_dim=1169, n_hid=400,
                                    T=5, H=8, L=2, norm=False)),
                   ("mag4_gnn4", dict(schema="mag", n_seed=128, width=128, depth=6, feat_dim=129, mean_degree=4.0, seed=3, in_dim=129, n_hid=512,
                                      T=4, H=8, L=4, norm=True))):
        batch = synthetic_sampled_batch(c["schema"], n_seed=c["n_seed"], width=c["width"], depth=c["depth"], feat_dim=c["feat_dim"],
                                        mean_degree=c["mean_degree"], seed=c["seed"])
        x, nt, tm, ei, et, _, ed = [t.to(dev) if torch.is_tensor(t) else t for t in to_torch_layout(*batch)]
        gnn = GNN(c["in_dim"], c["n_hid"], c["T"], len(ed), c["H"], c["L"], 0.2, "hgt", c["norm"], c["norm"], True, deterministic=DETERMINISTIC).to(dev).train()
        res[key] = {"N": int(nt.numel()), "E": int(et.numel()), "n_hid": c["n_hid"], "layers": c["L"],
                    "fwd_bwd_us": step_us(lambda: gnn(x, nt, tm, ei, et), list(gnn.parameters()), module=gnn)}
    res["optimizer"] = OPTIMIZER
    return res


def stacked_step(dev, Bs, out_path=None):
    """ms per piece of the sampled-size training step (forward + backward, dropout on, gradients dropped) on B stacked batches and on
    the same B batches one after the other; windows of the two interleaved, median of 5."""
    import statistics
    from pyhgt_amd import GNN
    from pyhgt_amd.sampled import stack_device_graphs, synthetic_sampled_batch, to_device_graph
    GraphPlan.CACHE_SIZE = 2 * max(Bs) + 8
    res = {"stack": list(Bs), "unit": "ms per piece (median of 5 alternating windows)", "deterministic": DETERMINISTIC}
    shapes = {"c3_layer": dict(schema="mag", n_seed=128, width=128, depth=6, feat_dim=256, mean_degree=4.0, seed=3),
              "c5_gnn2": dict(schema="oag", n_seed=256, width=128, depth=6, feat_dim=1169, mean_degree=1.2, seed=5)}

    def window(fn, params, iters):
        for it in range(2 + iters):
            if it == 2:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            for out in fn():
                out.backward(torch.ones_like(out))
            for p_ in params:
                p_.grad = None
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    for key, c in shapes.items():
        pieces = [to_device_graph(*synthetic_sampled_batch(c["schema"], n_seed=c["n_seed"], width=c["width"], depth=c["depth"],
                                                           feat_dim=c["feat_dim"], mean_degree=c["mean_degree"], seed=c["seed"] + i),
                                  device=dev) for i in range(max(Bs))]
        T, R = len(pieces[0][5]), len(pieces[0][6])
        if key == "c3_layer":
            model = HGTConv(256, 256, T, R, 8, 0.2, True, True, deterministic=DETERMINISTIC).to(dev).train()
            call = lambda g, x: model(x, g[1], g[3], g[4], g[2], plan=g.plan)
            leaf = lambda g: g[0].clone().requires_grad_(True)          # dx is part of the layer step, as in sampled_batches()
        else:
            model = GNN(1169, 400, T, R, 8, 2, 0.2, "hgt", False, False, True, deterministic=DETERMINISTIC).to(dev).train()
            call = lambda g, x: model(x, g[1], g[2], g[3], g[4])
            leaf = lambda g: g[0]
        params = list(model.parameters())
        res[key] = {"N_piece": int(pieces[0][1].numel()), "E_piece": int(pieces[0][4].numel())}
        for B in Bs:
            S, part = stack_device_graphs(pieces[:B]), pieces[:B]
            xS, xs = leaf(S), [leaf(g) for g in part]
            fns = [lambda: [call(S, xS)], lambda: [call(g, x) for g, x in zip(part, xs)]]
            leaves = [x for x in [xS] + xs if x.requires_grad]
            samples = [[], []]
            for _ in range(5):
                for i, fn in enumerate(fns):
                    samples[i].append(window(fn, params + leaves, max(4, 32 // B)))
            r = res[key]["B%d" % B] = {"N": int(S[1].numel()), "E": int(S[4].numel()),
                                       "stacked_ms": statistics.median(samples[0]) / B, "loop_ms": statistics.median(samples[1]) / B}
            print("%s x %2d  N=%6d E=%7d: training step stacked %.3f ms / piece, one after the other %.3f" % (key, B, r["N"], r["E"],
                                                                                                          r["stacked_ms"], r["loop_ms"]), flush=True)
            del S
        del pieces, model
        GraphPlan.clear_cache()
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return res


def emulated_rank_step(dev, W, out_path=None, iters=5):
    """One layer's training step of rank 0 of W (sizes of BASELINE.json configs[3] per rank, like bench.py --emulate-world): medians
    of `iters` steps from events on the compute stream.  return_ms is HaloPlan.return_grads inside the backward (the reverse
    transfers, emulated by device copies, + hgt_scatter_add_rows); link time is not part of any figure."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from pyhgt_amd.dist import HaloPlan, PartitionedGraph, target_blocks
    Nl, El, d, T, R, H, blocks = (int(os.environ.get("HGT_TRAIN_N", 1000000)), int(os.environ.get("HGT_TRAIN_E", 10000000)),
                                  int(os.environ.get("HGT_TRAIN_D", 256)), 4, 8, int(os.environ.get("HGT_TRAIN_H", 8)), 8)
    share, nt_g = bench.configs3_share(dev, W, 0, Nl, El, T, R, False, 0.0, 0.0, keep_global_types=True)
    n_own = int(share["node_type_own"].numel())
    bounds = target_blocks(share["dst_local"], n_own, blocks)
    eblock = torch.searchsorted(torch.tensor(bounds[1:], device=dev), share["dst_local"], right=True).clamp(max=blocks - 1)
    hp = HaloPlan(share["node_type_own"], share["src_global"], share["node_offsets"], 0, W, n_chunks=blocks, edge_block=eblock,
                  emulate={"node_type_global": nt_g})
    del nt_g, eblock
    pg = PartitionedGraph(None, None, share["dst_local"], share["edge_type"], None, T, R, Nl, 0, W, node_offsets=share["node_offsets"],
                          halo=hp, mode="blocked", n_chunks=blocks)
    torch.manual_seed(0)
    layer = HGTConv(d, d, T, R, H, 0.2, True, False, precision="bf16x3", deterministic=DETERMINISTIC).to(dev).train()
    x_own = torch.randn(n_own, d, device=dev, generator=torch.Generator(device=dev).manual_seed(7)).requires_grad_(True)
    g = torch.randn(n_own, d, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    marks = {}
    real_return = hp.return_grads

    def timed_return(*a, **k):      # events around the return path, on the stream the backward runs on
        marks["r0"], marks["r1"] = ev(), ev()
        marks["r0"].record()
        out = real_return(*a, **k)
        marks["r1"].record()
        return out
    hp.return_grads = timed_return
    rows = []
    for it in range(2 + iters):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        out = pg.forward(layer, x_own)
        e1.record()
        out.backward(g)
        e2.record()
        torch.cuda.synchronize()
        if it >= 2:
            rows.append((e0.elapsed_time(e1), e1.elapsed_time(e2), marks["r0"].elapsed_time(marks["r1"])))
        layer.zero_grad(set_to_none=True)
        x_own.grad = None
    med = lambda i: sorted(r[i] for r in rows)[len(rows) // 2]
    res = {"emulated_world": W, "rank": 0, "own_rows": n_own, "halo_rows": int(hp.n_halo), "returned_rows": int(hp.send_rows.numel()),
           "edges": int(share["dst_local"].numel()), "d": d, "H": H, "precision": "bf16x3", "deterministic": DETERMINISTIC,
           "training_forward_ms": round(med(0), 3), "backward_ms": round(med(1), 3), "return_ms": round(med(2), 3),
           "steps": iters, "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
           "note": "forward = exchange (device copies) + rectangular step; backward includes return_ms = reverse transfers (device "
                   "copies) + hgt_scatter_add_rows; medians of events on the compute stream"}
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")
    return res


def recompute_compare(dev, out_path=None, warmup=5, iters=20):
    """The memory-lean training mode against the default one (see the module docstring)."""
    from pyhgt_amd import _lib
    N, E, d, T, R, H = (int(os.environ.get("HGT_TRAIN_N", 1000000)), int(os.environ.get("HGT_TRAIN_E", 10000000)),
                        int(os.environ.get("HGT_TRAIN_D", 256)), 4, 8, int(os.environ.get("HGT_TRAIN_H", 8)))
    x, nt, ei, et, tm = [t.to(dev) for t in synthetic_typed_graph(N, E, d, T, R, seed=1)]
    plan = GraphPlan(nt, ei, et, None, T, R)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    med = lambda v: sorted(v)[len(v) // 2]
    torch.manual_seed(0)
    layers = {m: HGTConv(d, d, T, R, H, 0.2, True, False, deterministic=DETERMINISTIC, recompute=(m == "recompute")).to(dev).train()
              for m in ("default", "recompute")}
    layers["recompute"].load_state_dict(layers["default"].state_dict())
    xg = x.clone().requires_grad_(True)
    g = torch.randn(N, d, device=dev)
    rows = {m: [] for m in layers}
    for it in range(warmup + iters):
        for m, layer in layers.items():                            # the two modes alternate: both see the same clocks
            e0, e1, e2 = ev(), ev(), ev()
            e0.record()
            out = layer(xg, nt, ei, et, None, plan=plan)
            e1.record()
            out.backward(g)
            e2.record()
            torch.cuda.synchronize()
            if it >= warmup:
                rows[m].append((e0.elapsed_time(e1), e1.elapsed_time(e2), e0.elapsed_time(e2)))
            layer.zero_grad(set_to_none=True)
            xg.grad = None
            del out
    res = {"N": N, "E": E, "d": d, "H": H, "dropout": 0.2, "deterministic": DETERMINISTIC, "warmup": warmup, "steps": iters}
    for m in layers:
        res[m] = {k: round(med([r[i] for r in rows[m]]), 3) for i, k in enumerate(("forward_ms", "backward_ms", "step_ms"))}
        res[m]["step_ms_min_max"] = [round(min(r[2] for r in rows[m]), 3), round(max(r[2] for r in rows[m]), 3)]
    res["step_ratio_recompute_over_default"] = round(res["recompute"]["step_ms"] / res["default"]["step_ms"], 4)
    del layers, xg, g
    # peak memory of a four-layer step, one mode after the other
    for m in ("default", "recompute"):
        stack = [HGTConv(d, d, T, R, H, 0.2, True, False, deterministic=DETERMINISTIC, recompute=(m == "recompute")).to(dev).train()
                 for _ in range(4)]
        xg = x.clone().requires_grad_(True)
        for it in range(2):
            if it == 1:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
            h = xg
            for layer in stack:
                h = layer(h, nt, ei, et, None, plan=plan)
            torch.cuda.synchronize()
            kept = torch.cuda.memory_allocated()
            h.backward(torch.ones_like(h))
            torch.cuda.synchronize()
            for layer in stack:
                layer.zero_grad(set_to_none=True)
            xg.grad = None
            del h
        res[m]["four_layer_step"] = {"max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 1e9, 3),
                                     "kept_after_forward_gb": round((kept - base) / 1e9, 3),
                                     "allocated_before_gb": round(base / 1e9, 3)}
        del stack, xg
    del x, nt, ei, et, tm, plan
    GraphPlan.clear_cache()
    torch.cuda.empty_cache()
    # the dropout kernel alone: apply (reads and writes x) against mul_inplace (reads x and a mask, writes x)
    lib, n = _lib.load(), 1 << 28
    st = torch.cuda.current_stream().cuda_stream
    a = torch.randn(n, device=dev)
    mask = torch.empty(n, device=dev)
    _lib.check(lib.hgt_dropout_mask(mask.data_ptr(), n, 12345, 0, 0.8, st), "hgt_dropout_mask")
    calls = {"hgt_dropout_apply": lambda: lib.hgt_dropout_apply(a.data_ptr(), n, 12345, 0, 0.8, st),
             "hgt_mul_inplace": lambda: lib.hgt_mul_inplace(a.data_ptr(), mask.data_ptr(), n, st),
             "hgt_dropout_mask": lambda: lib.hgt_dropout_mask(mask.data_ptr(), n, 12345, 0, 0.8, st)}
    times = {k: [] for k in calls}
    for it in range(warmup + iters):
        for k, fn in calls.items():
            e0, e1 = ev(), ev()
            e0.record()
            _lib.check(fn(), k)
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append(e0.elapsed_time(e1))
    moved = {"hgt_dropout_apply": 8 * n, "hgt_mul_inplace": 12 * n, "hgt_dropout_mask": 4 * n}
    res["dropout_kernels"] = {"n": n, **{k: {"ms": round(med(v), 4), "gb_per_s": round(moved[k] / (med(v) * 1e-3) / 1e9, 1)}
                                         for k, v in times.items()}}
    res["dropout_kernels"]["apply_over_mul_inplace"] = round(med(times["hgt_dropout_apply"]) / med(times["hgt_mul_inplace"]), 4)
    line = json.dumps(res, indent=1)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return res


def trim_step(dev, Bs, papers, out_path=None, only=None):
    """--trim: the training step (forward + backward of the seed rows, dropout on, gradients dropped) untrimmed against trimmed
    (GNN.forward(seeds=): the trim and its plan builds inside the timed step), on the workloads and models of tools/bench_small.py
    --trim, and peak / kept memory of a step of the 4-layer model in both forms."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_small import alternating_spread, merge_out, trim_cases, trim_shares, trim_verdict
    from pyhgt_amd import GNN, trim_to_seeds
    res = {"papers": papers, "seeds": 128, "depth": 6, "deterministic": DETERMINISTIC, "cases": [],
           "unit": "us per step: median, min and max of 5 alternating windows of ~0.3 s; memory in MB above what was allocated before the step"}
    for name, B, g, rows, m in trim_cases(dev, papers, Bs, only):
        T, R, L = len(g[5]), len(g[6]), m["L"]
        gnn = GNN(m["in_dim"], m["n_hid"], T, R, m["H"], L, 0.2, "hgt", m["norm"], m["norm"], True, deterministic=DETERMINISTIC).to(dev).train()
        params = list(gnn.parameters())

        def step(trimmed):
            out = gnn(g[0], g[1], g[2], g[3], g[4], seeds=rows) if trimmed else gnn(g[0], g[1], g[2], g[3], g[4])[rows]
            out.backward(torch.ones_like(out))
            for p_ in params:
                p_.grad = None
        u, t = alternating_spread([lambda: step(False), lambda: step(True)])
        case = {"workload": name, "B": B, "layers": L, "n_hid": m["n_hid"], **trim_shares(trim_to_seeds(g, rows, L), g[1].numel(), g[4].numel()),
                "untrimmed": u, "trimmed": t, **trim_verdict(u, t)}
        if L == 4:
            for key, trimmed in (("untrimmed", False), ("trimmed", True)):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                out = gnn(g[0], g[1], g[2], g[3], g[4], seeds=rows) if trimmed else gnn(g[0], g[1], g[2], g[3], g[4])[rows]
                torch.cuda.synchronize()
                kept = torch.cuda.memory_allocated() - base
                out.backward(torch.ones_like(out))
                torch.cuda.synchronize()
                case[key]["kept_after_forward_mb"] = round(kept / 1e6, 2)
                case[key]["peak_mb"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 2)
                del out
                for p_ in params:
                    p_.grad = None
        res["cases"].append(case)
        print("%s x %2d  %d layers: training step untrimmed %.0f us [%.0f, %.0f], trimmed %.0f us [%.0f, %.0f], pays: %s%s"
              % (name, B, L, u["median_us"], u["min_us"], u["max_us"], t["median_us"], t["min_us"], t["max_us"], case["pays"],
                 "" if L != 4 else ", peak %.1f -> %.1f MB, kept %.1f -> %.1f MB" % (u["peak_mb"], t["peak_mb"], u["kept_after_forward_mb"],
                                                                                 t["kept_after_forward_mb"])), flush=True)
        del gnn, params
    merge_out(out_path, "training_step", res)
    return res


def main():
    dev = "cuda:0"
    if "--trim" in sys.argv:
        arg = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
        trim_step(dev, [int(v) for v in arg("--batches", "1,16").split(",")], int(arg("--papers", "50000")), arg("--out", None), arg("--only", None))
        return
    if "--recompute" in sys.argv:
        recompute_compare(dev, sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None)
        return
    if "--stack" in sys.argv:
        stacked_step(dev, [int(v) for v in sys.argv[sys.argv.index("--stack") + 1].split(",")],
                     sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None)
        return
    if "--emulate-world" in sys.argv:
        W = int(sys.argv[sys.argv.index("--emulate-world") + 1])
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
        emulated_rank_step(dev, W, out)
        return
    # HGT_TRAIN_D / HGT_TRAIN_H: layer width and head count (defaults: configs[1]; 768 / 8 and 1024 / 8 are the wide-head layouts)
    N, E, d, T, R, H = (int(os.environ.get("HGT_TRAIN_N", 1000000)), int(os.environ.get("HGT_TRAIN_E", 10000000)),
                        int(os.environ.get("HGT_TRAIN_D", 256)), 4, 8, int(os.environ.get("HGT_TRAIN_H", 8)))
    x, nt, ei, et, tm = [t.to(dev) for t in synthetic_typed_graph(N, E, d, T, R, seed=1)]
    layer = HGTConv(d, d, T, R, H, 0.2, True, False, deterministic=DETERMINISTIC).to(dev)
    plan = GraphPlan(nt, ei, et, None, T, R)
    res = {}
    layer.eval()
    with torch.no_grad():
        for _ in range(3):
            layer(x, nt, ei, et, None, plan=plan)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            layer(x, nt, ei, et, None, plan=plan)
        torch.cuda.synchronize()
        res["inference_forward_ms"] = (time.perf_counter() - t0) / 10 * 1e3
    layer.train()
    xg = x.clone().requires_grad_(True)
    g = torch.randn(N, d, device=dev)
    iters = 5 if N >= 200000 else 50          # a sampled-batch-sized graph steps in ~2 ms: time enough of them
    for phase in ("forward_ms", "forward_backward_ms"):
        for it in range(2 + iters):
            if it == 2:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            out = layer(xg, nt, ei, et, None, plan=plan)
            if phase == "forward_backward_ms":
                out.backward(g)
                layer.zero_grad(set_to_none=True)
                xg.grad = None
        torch.cuda.synchronize()
        res["training_" + phase] = (time.perf_counter() - t0) / iters * 1e3
    res["N"], res["E"], res["d"], res["H"] = N, E, d, H
    res["deterministic"] = DETERMINISTIC
    res["peak_mem_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
    fwd_b, bwd_b = training_step_bytes(N, E, d, H)
    bf, bb = sum(fwd_b.values()), sum(bwd_b.values())
    t_f, t_s = res["training_forward_ms"], res["training_forward_backward_ms"]
    mb = minimal_backward_bytes(N, E, d, H)
    res["roofline"] = {
        "bound": "hbm", "peak": 8000.0, "unit": "GB/s",
        "algorithmic_bytes": {"training_forward": bf, "backward": bb, "step": bf + bb},
        # against a minimal-traffic backward (four gather passes) instead of the kernels as built (seven): the stricter figure
        "minimal_backward_bytes": sum(mb.values()), "minimal_backward_bytes_by_part": mb,
        "backward_frac_of_minimal_model": round(sum(mb.values()) / ((res["training_forward_backward_ms"] - res["training_forward_ms"]) * 1e-3) / 1e9 / 8000.0, 4),
        "achieved": round((bf + bb) / (t_s * 1e-3) / 1e9, 1), "frac": round((bf + bb) / (t_s * 1e-3) / 1e9 / 8000.0, 4),
        "training_forward_frac": round(bf / (t_f * 1e-3) / 1e9 / 8000.0, 4),
        "backward_frac": round(bb / ((t_s - t_f) * 1e-3) / 1e9 / 8000.0, 4),
        "backward_bytes_by_kernel": bwd_b, "training_forward_bytes_by_kernel": fwd_b,
        "note": "per-kernel times: rocprofv3 kernel statistics of this command (tools/profile_train.sh -> profiles/<tag>_train_kernel_stats.txt)"}
    if not os.environ.get("HGT_TRAIN_NO_SMALL"):
        del x, xg, g, layer, plan
        torch.cuda.empty_cache()
        res["sampled_batches"] = sampled_batches(dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
