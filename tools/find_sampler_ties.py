#!/usr/bin/env python3
"""Search for a neighbour-subset draw of the device sampler whose threshold word is duplicated (numpy only, no GPU).

A row (target id, meta triple, step) with more than sampled_number neighbours keeps the sampled_number smallest
(Philox word, position) pairs, word = philox4x32_10(position, target id, step, 0x10000 + triple, seed)[0].  When the r-th and the
(r + 1)-th smallest words of a row are equal, a draw with sampled_number = r has to break the tie by position: the branch of
`budget_row` (csrc/hgt_sampler.hip) that bisects on the position.  For 32-bit words that happens about once in 2^33 / degree^2 rows, so
no random test graph has such a row; this tool finds one, and tests/test_sampler.py keeps what it found (TIES).

    python tools/find_sampler_ties.py --degree 60000 --max-r 1023                 # a workgroup's row: ~1 s
    python tools/find_sampler_ties.py --degree 512 --targets 4096 --seeds 64      # a wavefront's row: ~1 in 3 * 10^4 rows

Prints one line per tie: seed, target id, step, triple index, degree, r (1-based: the r-th and (r + 1)-th smallest words are equal),
the word and the two positions that hold it."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyhgt_amd.sampler import philox4x32_10, _SUBSET_TAG  # noqa: E402


def row_words(degree, target, step, triple, seed):
    """the words of one row, by position"""
    return philox4x32_10(np.arange(degree), target, step, _SUBSET_TAG + triple, seed)[0]


def tie_of_row(words, max_r):
    """-> (r, word, position of the r-th, position of the (r + 1)-th smallest (word, position)) of the first tie with r <= max_r, or None"""
    order = np.lexsort((np.arange(words.size), words))
    w = words[order][:max_r + 1]
    hit = np.nonzero(w[1:] == w[:-1])[0]
    if hit.size == 0:
        return None
    i = int(hit[0])
    return i + 1, int(w[i]), int(order[i]), int(order[i + 1])


def search(degree, max_r, seeds, targets, step, triple, chunk=1 << 22):
    """every (seed, target) row of `degree` words; yields (seed, target, step, triple, degree, r, word, p, p')"""
    per = max(1, chunk // degree)
    pos = np.arange(degree)[None, :]
    for seed in seeds:
        for t0 in range(targets[0], targets[1], per):
            tg = np.arange(t0, min(targets[1], t0 + per))
            w = np.sort(philox4x32_10(pos, tg[:, None], step, _SUBSET_TAG + triple, seed)[0], axis=1)[:, :max_r + 1]
            for row in np.nonzero((w[:, 1:] == w[:, :-1]).any(axis=1))[0]:
                target = int(tg[row])
                r, word, p, q = tie_of_row(row_words(degree, target, step, triple, seed), max_r)
                yield seed, target, step, triple, degree, r, word, p, q


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--degree", type=int, default=60000, help="neighbours of the row")
    ap.add_argument("--max-r", type=int, default=None, help="largest r reported (default: min(degree - 2, 1023), so that "
                    "sampled_number = r and r + 1 both draw)")
    ap.add_argument("--seeds", type=int, default=64, help="seeds 0 .. SEEDS - 1")
    ap.add_argument("--targets", type=int, default=128, help="target ids 0 .. TARGETS - 1")
    ap.add_argument("--step", type=int, default=0)
    ap.add_argument("--triple", type=int, default=0)
    ap.add_argument("--all", action="store_true", help="do not stop at the first tie")
    a = ap.parse_args()
    max_r = min(a.degree - 2, 1023) if a.max_r is None else a.max_r
    t0, n = time.time(), 0
    for hit in search(a.degree, max_r, range(a.seeds), (0, a.targets), a.step, a.triple):
        n += 1
        print("seed %d  target %d  step %d  triple %d  degree %d  r %d  word 0x%08x  positions %d, %d  (%.1f s)" % (hit + (time.time() - t0,)))
        if not a.all:
            break
    if n == 0:
        print("no tie among %d rows of %d words (%.1f s)" % (a.seeds * a.targets, a.degree, time.time() - t0))


if __name__ == "__main__":
    main()
