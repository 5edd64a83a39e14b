#!/usr/bin/env python
"""tools/bench_halo_return.py: the reduce kernel of the gradient return path (hgt_scatter_add_rows) next to the forward's pack kernel
(hgt_gather_rows) at the size of a rank of 8: 1 M own rows, ~5 M halo rows of d floats, the multiplicities of the rows drawn as
HaloPlan(emulate=...) draws its send list (uniformly from the own rows).  Two rates per kernel, GB/s over
  * "bytes": every access the kernel makes -- gather: a read and a write per sent row (its reads hit only `own` DISTINCT rows, each
    about halo / own times, so most of them can be served by the caches: this is a traffic rate, not an HBM rate); scatter-add: a
    read per received row + a read and a write per destination row that receives something (every byte is touched once);
  * "unique_bytes": distinct bytes, what HBM must deliver at the least -- gather: the distinct source rows once + every packed row
    written; scatter-add: the same as "bytes".
Warm-up rounds, then `--repeats` rounds in which the two kernels ALTERNATE (gather, scatter-add, gather, ...), each call between
its own pair of events, so that clock and cache state drift hits both alike; median, 10th and 90th percentile per kernel.  The
default 200 rounds keep each kernel busy for some 0.3 s.

    python tools/bench_halo_return.py [--own 1000000] [--halo 5000000] [--d 256] [--out profiles/r08_halo_return.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd import _lib  # noqa: E402
from pyhgt_amd.dist import HaloPlan  # noqa: E402


def timed_alternating(fns, warmup, repeats):
    """fns: {name: callable}.  Rounds of one call each, in the given order; per name the sorted times of its calls."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    marks = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            marks[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, evs in marks.items():
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        out[k] = dict(median_ms=ms[len(ms) // 2], p10_ms=ms[len(ms) // 10], p90_ms=ms[(9 * len(ms)) // 10], repeats=repeats,
                      busy_ms=sum(ms))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--own", type=int, default=1_000_000)
    ap.add_argument("--halo", type=int, default=5_000_000)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(977)
    hp = HaloPlan.__new__(HaloPlan)                       # the send side alone: rows drawn like HaloPlan(emulate=...)
    hp.send_rows = torch.randint(0, a.own, (a.halo,), generator=g, device=dev).to(torch.int32)
    rows, ptr, pos = hp.return_index(dev)
    n_rows, d = int(rows.numel()), a.d
    recv = torch.randn(a.halo, d, device=dev)
    d_own = torch.randn(a.own, d, device=dev)
    packed = torch.empty(a.halo, d, device=dev)

    def scatter():
        _lib.check(lib.hgt_scatter_add_rows(recv.data_ptr(), d, rows.data_ptr(), ptr.data_ptr(), pos.data_ptr(), n_rows, d,
                                            d_own.data_ptr(), d, st), "hgt_scatter_add_rows")

    def gather():
        _lib.check(lib.hgt_gather_rows(d_own.data_ptr(), d, hp.send_rows.data_ptr(), a.halo, d, packed.data_ptr(), st), "hgt_gather_rows")

    res = dict(own_rows=a.own, halo_rows=a.halo, d=d, destination_rows=n_rows, max_multiplicity=int((ptr[1:] - ptr[:-1]).max()))
    n_src = int(torch.unique(hp.send_rows).numel())      # distinct rows the gather reads
    nbytes = {"hgt_gather_rows": (2 * a.halo * d * 4, (n_src + a.halo) * d * 4),
              "hgt_scatter_add_rows": ((a.halo + 2 * n_rows) * d * 4, (a.halo + 2 * n_rows) * d * 4)}
    res["interleaved"] = True
    for name, t in timed_alternating({"hgt_gather_rows": gather, "hgt_scatter_add_rows": scatter}, a.warmup, a.repeats).items():
        t["bytes"], t["unique_bytes"] = nbytes[name]
        t["gb_per_s"] = t["bytes"] / t["median_ms"] / 1e6
        t["unique_gb_per_s"] = t["unique_bytes"] / t["median_ms"] / 1e6
        res[name] = t
    line = json.dumps(res)
    print(line)
    if a.out:      # (one JSON object per line: tools/bench_train.py --emulate-world appends its line to the same file)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
