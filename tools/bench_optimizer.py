#!/usr/bin/env python
"""The optimizer step alone, on the parameter sets this project trains: clip_grad_norm_ + torch.optim.AdamW (default foreach), the same
with fused=True, and pyhgt_amd.AdamW(max_norm=...) -- alternating in ONE process on the same shapes, torch as the comparator in the same run.

    python tools/bench_optimizer.py [--steps 200] [--warmup 20] [--repeats 3] [--out profiles/r18_optimizer_step.json]
    python tools/bench_optimizer.py --only device --model oag4x400 --steps 50      # one contender: for rocprofv3 --kernel-trace --stats

Per model (a GNN plus its Classifier) and contender: fresh gradient tensors are assigned before every step, as zero_grad() + backward
leave them, so the gradient pointers change each step; a host clock around `steps` steps that end in one synchronise, after a
warm-up; the median and the spread (min, max) over `repeats` windows.  floor_us is the time the 28 + 4 bytes per element of the update
and the norm take at 5 TB/s -- a figure from shapes, not a measurement."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pyhgt_amd  # noqa: E402
from pyhgt_amd import GNN, Classifier  # noqa: E402

MODELS = {      # GNN arguments (in_dim, n_hid, types, relations, heads, layers) and the Classifier's classes
    "c3_layer": ((256, 256, 4, 8, 8, 1), 16),
    "oag4x400": ((1169, 400, 5, 33, 8, 4), 16),
    "mag4x512": ((129, 512, 4, 8, 8, 4), 349),
}
CLIP = 0.5


def contenders(params):
    def torch_pair(**kw):
        opt = torch.optim.AdamW(params, lr=1e-3, **kw)
        return lambda: (torch.nn.utils.clip_grad_norm_(params, CLIP), opt.step())
    return {"torch_foreach": lambda: torch_pair(), "torch_fused": lambda: torch_pair(fused=True),
            "device": lambda: pyhgt_amd.AdamW(params, lr=1e-3, max_norm=CLIP).step}


def window(step, params, pool, steps):
    """us per step: `steps` steps, each on the gradient tensors of another slot of the pool, one synchronise at the end"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(steps):
        for p, g in zip(params, pool[it % len(pool)]):
            p.grad = g
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["torch_foreach", "torch_fused", "device"])
    ap.add_argument("--model", default=None, choices=list(MODELS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    res = {"steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "clip": CLIP, "torch": torch.__version__,
           "device_name": torch.cuda.get_device_name(0), "models": {}}
    for name, (gnn_args, n_cls) in MODELS.items():
        if a.model and name != a.model:
            continue
        torch.manual_seed(0)
        model = torch.nn.ModuleList([GNN(*gnn_args, dropout=0.2, prev_norm=False, last_norm=False, use_RTE=True),
                                     Classifier(gnn_args[1], n_cls)]).to(dev)
        params = list(model.parameters())
        numel = sum(p.numel() for p in params)
        pool = [[torch.randn_like(p) * 1e-2 for p in params] for _ in range(3)]           # three sets of gradient tensors: other pointers each step
        row = {"tensors": len(params), "elements": numel, "floor_us": round(numel * 32 / 5e12 * 1e6, 1), "us_per_step": {}}
        made = {}
        for k, make in contenders(params).items():
            if a.only in (None, k):
                try:
                    made[k] = make()
                except (RuntimeError, ValueError) as e:                                    # e.g. fused=True where this build lacks it
                    row["us_per_step"][k] = {"unavailable": str(e).splitlines()[0]}
        for step in made.values():
            window(step, params, pool, a.warmup)
        times = {k: [] for k in made}
        for _ in range(a.repeats):                                                         # alternating: every contender once per repeat
            for k, step in made.items():
                times[k].append(window(step, params, pool, a.steps))
        for k, v in times.items():
            v = sorted(v)
            row["us_per_step"][k] = {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}
        res["models"][name] = row
        print(name, json.dumps(row), flush=True)
        del model, params, pool, made
        torch.cuda.empty_cache()
    line = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
