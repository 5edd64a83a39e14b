"""CPU tests of the batched device sampler (sample_subgraphs_device / sample_subgraphs_host, the hgt_sampler_*_batched entry points):
the argument rules of the new C entry points, called through ctypes on host buffers so that every call must return before it
launches anything, the host definition as the list of the single host calls, and the shape rules of a batched call.  No kernel runs
here; tests/test_batched_sampler_gpu.py runs the batched calls on the device."""
import ctypes as C

import numpy as np
import pytest

import test_sampler as TS
from pyhgt_amd import _lib, sample_subgraphs_device, sample_subgraphs_host
from pyhgt_amd.sampler import sample_subgraph_host

INV, UNS, WS, BIG = -1, -2, -3, -4


def test_batch_limit_is_exported():
    assert _lib.HGT_SAMPLER_MAX_BATCH >= 16
    text = open(TS.os.path.join(TS.ROOT, "include", "hgt_hip.h")).read()
    assert "#define HGT_SAMPLER_MAX_BATCH %d\n" % _lib.HGT_SAMPLER_MAX_BATCH in text


def test_batched_abi_argument_rules():
    lib = _lib.load()
    buf, p, types, triples = TS._tables()                     # 2 types of 8 nodes, lists of 4 / 8, 2 triples: 8 induce slots
    over = _lib.HGT_SAMPLER_MAX_BATCH + 1
    seeds = (C.c_uint64 * over)(*range(over))
    # seed: (types, T, B, type, ids, times, n, step, stream)
    assert lib.hgt_sampler_seed_batched(types, 2, 0, 0, p, p, 2, 0, None) == INV
    assert lib.hgt_sampler_seed_batched(types, 2, -3, 0, p, p, 2, 0, None) == INV
    assert lib.hgt_sampler_seed_batched(types, 2, over, 0, p, p, 2, 0, None) == UNS
    assert lib.hgt_sampler_seed_batched(None, 2, 2, 0, p, p, 2, 0, None) == INV
    assert lib.hgt_sampler_seed_batched(types, 2, 2, 0, None, p, 2, 0, None) == INV
    assert lib.hgt_sampler_seed_batched(types, 2, 2, 0, p, None, 2, 0, None) == INV
    assert lib.hgt_sampler_seed_batched(types, 2, 2, 0, p, p, -1, 0, None) == INV
    assert lib.hgt_sampler_seed_batched(types, 2, 2, 2, p, p, 2, 0, None) == INV
    assert lib.hgt_sampler_seed_batched(types, 2, 2, 0, p, p, 5, 0, None) == WS
    # add_budget: (types, T, triples, M, B, type, step, sampled_number, max_new, has_max, max_time, seeds, hub, hub_entries, stream)
    assert lib.hgt_sampler_add_budget_batched(types, 2, triples, 2, 0, 0, 0, 4, 2, 0, 0, seeds, p, 64, None) == INV
    assert lib.hgt_sampler_add_budget_batched(types, 2, triples, 2, over, 0, 0, 4, 2, 0, 0, seeds, p, 64, None) == UNS
    assert lib.hgt_sampler_add_budget_batched(types, 2, triples, 2, 2, 0, 0, 4, 2, 0, 0, None, p, 64, None) == INV
    assert lib.hgt_sampler_add_budget_batched(types, 2, triples, 2, 2, 0, 0, 4, 2, 0, 0, seeds, None, 64, None) == INV
    assert lib.hgt_sampler_add_budget_batched(types, 2, triples, 2, 2, 0, 0, 4, 2, 0, 0, seeds, p, 2, None) == WS       # 2 rows + 1 per replica
    assert lib.hgt_sampler_add_budget_batched(types, 2, triples, 2, 2, 0, 0, 4, -2, 0, 0, seeds, p, 64, None) == INV
    assert lib.hgt_sampler_add_budget_batched(types, 2, triples, 2, 2, 0, 0, 0, 2, 0, 0, seeds, p, 64, None) == INV
    assert lib.hgt_sampler_add_budget_batched(types, 2, triples, 2, 2, 0, 0, _lib.HGT_SAMPLER_MAX_NUMBER + 1, 2, 0, 0, seeds, p, 64, None) == UNS
    assert lib.hgt_sampler_add_budget_batched(types, 2, None, 2, 2, 0, 0, 4, 2, 0, 0, seeds, p, 64, None) == INV
    assert lib.hgt_sampler_add_budget_batched(types, 2, triples, 2, 2, 0, 0, 4, 0, 0, 0, seeds, None, 0, None) == 0       # no row: nothing to do
    # select: (types, T, B, type, step, sampled_number, seeds, keys, tmp, tmp_entries, stream)
    assert lib.hgt_sampler_select_batched(types, 2, 0, 0, 0, 4, seeds, p, p, 8, None) == INV
    assert lib.hgt_sampler_select_batched(types, 2, over, 0, 0, 4, seeds, p, p, 8, None) == UNS
    assert lib.hgt_sampler_select_batched(types, 2, 2, 0, 0, 4, None, p, p, 8, None) == INV
    assert lib.hgt_sampler_select_batched(types, 2, 2, 0, 0, 4, seeds, None, p, 8, None) == INV
    assert lib.hgt_sampler_select_batched(types, 2, 2, 0, 0, 4, seeds, p, None, 8, None) == INV
    assert lib.hgt_sampler_select_batched(types, 2, 2, 0, 0, 4, seeds, p, p, 7, None) == WS
    assert lib.hgt_sampler_select_batched(types, 2, 2, -1, 0, 4, seeds, p, p, 8, None) == INV
    # induce, count pass: (types, T, triples, M, B, R, rowoff, hub, n_entries, type_off, rel_ptr, sizes[, masks], stream)
    masks = (_lib.HgtSamplerMask * 2)()
    for count, tail in ((lib.hgt_sampler_induce_count_batched, ()), (lib.hgt_sampler_induce_count_masked_batched, (masks,))):
        assert count(types, 2, triples, 2, 0, 3, p, p, 9, p, p, p, *tail, None) == INV
        assert count(types, 2, triples, 2, over, 3, p, p, 9, p, p, p, *tail, None) == UNS
        assert count(types, 2, triples, 2, 2, 3, p, p, 8, p, p, p, *tail, None) == WS                  # 8 slots + 1 per replica
        assert count(types, 2, triples, 2, 2, 3, None, p, 9, p, p, p, *tail, None) == INV
        assert count(types, 2, triples, 2, 2, 3, p, None, 9, p, p, p, *tail, None) == INV
        assert count(types, 2, triples, 2, 2, 3, p, p, 9, p, p, None, *tail, None) == INV
        assert count(types, 2, triples, 2, 2, 2, p, p, 9, p, p, p, *tail, None) == INV                 # rel_id 1 is not below self = 1
    assert lib.hgt_sampler_induce_count_masked_batched(types, 2, triples, 2, 2, 3, p, p, 9, p, p, p, None, None) == INV
    bad = (_lib.HgtSamplerMask * 2)()
    bad[1].src_below = -1
    assert lib.hgt_sampler_induce_count_masked_batched(types, 2, triples, 2, 2, 3, p, p, 9, p, p, p, bad, None) == INV
    # fill pass: (..., B, R, rowoff, hub, n_entries, type_off, sizes, offs_out, n_nodes, n_edges, src, dst, time, node_time, node_id[, masks], stream)
    for fill, tail in ((lib.hgt_sampler_induce_fill_batched, ()), (lib.hgt_sampler_induce_fill_masked_batched, (masks,))):
        assert fill(types, 2, triples, 2, 0, 3, p, p, 9, p, p, p, 4, 6, p, p, p, p, p, *tail, None) == INV
        assert fill(types, 2, triples, 2, over, 3, p, p, 9, p, p, p, 4, 6, p, p, p, p, p, *tail, None) == UNS
        assert fill(types, 2, triples, 2, 2, 3, p, p, 8, p, p, p, 4, 6, p, p, p, p, p, *tail, None) == WS
        assert fill(types, 2, triples, 2, 2, 3, p, p, 9, p, None, p, 4, 6, p, p, p, p, p, *tail, None) == INV      # sizes
        assert fill(types, 2, triples, 2, 2, 3, p, p, 9, p, p, None, 4, 6, p, p, p, p, p, *tail, None) == INV      # offs_out
        assert fill(types, 2, triples, 2, 2, 3, p, p, 9, p, p, p, -1, 6, p, p, p, p, p, *tail, None) == INV
        assert fill(types, 2, triples, 2, 2, 3, p, p, 9, p, p, p, 4, 3, p, p, p, p, p, *tail, None) == INV         # fewer edges than self loops
        assert fill(types, 2, triples, 2, 2, 3, p, p, 9, p, p, p, 4, 6, None, p, p, p, p, *tail, None) == INV
        assert fill(types, 2, triples, 2, 2, 3, p, p, 9, p, p, p, 4, 6, p, p, p, p, None, *tail, None) == INV
        assert fill(types, 2, triples, 2, 2, 3, p, p, 9, p, p, p, 4, 2 ** 31, p, p, p, p, p, *tail, None) == BIG
    assert lib.hgt_sampler_induce_fill_masked_batched(types, 2, triples, 2, 2, 3, p, p, 9, p, p, p, 4, 6, p, p, p, p, p, None, None) == INV
    # reset: (types, T, B, stream)
    assert lib.hgt_sampler_reset_batched(types, 2, 0, None) == INV
    assert lib.hgt_sampler_reset_batched(types, 2, over, None) == UNS
    assert lib.hgt_sampler_reset_batched(None, 2, 2, None) == INV
    # gather_features: (features, rows per matrix, T, B, width, type_off, offs, node_id, n_nodes, out, stream)
    feats, rows = (C.c_void_p * 2)(p, p), (C.c_int32 * 2)(8, 8)
    assert lib.hgt_sampler_gather_features(None, rows, 2, 2, 4, p, p, p, 3, p, None) == INV
    assert lib.hgt_sampler_gather_features(feats, None, 2, 2, 4, p, p, p, 3, p, None) == INV
    assert lib.hgt_sampler_gather_features(feats, rows, 2, 0, 4, p, p, p, 3, p, None) == INV
    assert lib.hgt_sampler_gather_features(feats, rows, 2, over, 4, p, p, p, 3, p, None) == UNS
    assert lib.hgt_sampler_gather_features(feats, rows, _lib.HGT_SAMPLER_MAX_TYPES + 1, 2, 4, p, p, p, 3, p, None) == UNS
    assert lib.hgt_sampler_gather_features(feats, rows, 2, 2, -1, p, p, p, 3, p, None) == INV
    assert lib.hgt_sampler_gather_features(feats, rows, 2, 2, 4, p, p, p, -1, p, None) == INV
    assert lib.hgt_sampler_gather_features(feats, rows, 2, 2, 4, p, p, None, 3, p, None) == INV
    assert lib.hgt_sampler_gather_features(feats, rows, 2, 2, 4, p, None, p, 3, p, None) == INV
    assert lib.hgt_sampler_gather_features(feats, rows, 2, 2, 4, p, p, p, 3, None, None) == INV
    assert lib.hgt_sampler_gather_features(feats, (C.c_int32 * 2)(8, -1), 2, 2, 4, p, p, p, 3, p, None) == INV
    assert lib.hgt_sampler_gather_features(feats, rows, 2, 2, 4, None, None, None, 0, None, None) == 0      # no row: nothing to do
    del buf


def _group(inp, depth, sn):
    calls = [c for c in TS.OAG_CALLS if c[0] is inp and c[2:4] == (depth, sn)]
    assert len(calls) >= 2 and len({c[:4] == calls[0][:4] for c in calls}) == 1
    return calls


@pytest.mark.parametrize("inp, depth, sn", [(TS._PAPERS, 3, 16), (TS._THREE, 3, 128)], ids=["papers", "three"])
def test_host_definition_is_the_list_of_single_host_calls(inp, depth, sn):
    dg = TS.oag_graph()
    calls = _group(inp, depth, sn)
    got = sample_subgraphs_host(dg, calls[0][1], depth, sn, [c[0] for c in calls], [c[4] for c in calls])
    assert len(got) == len(calls)
    for res, (_, max_time, _, _, seed) in zip(got, calls):
        one = sample_subgraph_host(dg, max_time, depth, sn, inp, seed)
        assert all(np.array_equal(a, b) for a, b in zip(res.sorted, one.sorted))
        assert all(np.array_equal(res.indxs[t], one.indxs[t]) and np.array_equal(res.times[t], one.times[t]) for t in dg.types)
        assert all(a.dtype == b.dtype and a.equal(b) for a, b in zip(res[:5], one[:5])) and res.n_seed == one.n_seed
    assert any(not np.array_equal(got[0].indxs[t], got[1].indxs[t]) for t in dg.types)       # other Philox seeds, other draws


def test_batched_call_checks_its_shape_before_anything_else():
    """on a host graph: the shape errors come first, then the refusal of the single call"""
    dg = TS.oag_graph()
    a, b = {"paper": [[1, 0], [2, 0]]}, {"paper": [[3, 0]]}
    for fn in (sample_subgraphs_device, sample_subgraphs_host):
        with pytest.raises(ValueError):
            fn(dg, None, 1, 4, [a, a], [0])                  # len(seeds) != len(inps)
    with pytest.raises(ValueError, match="seeds per type"):
        sample_subgraphs_device(dg, None, 1, 4, [a, b], [0, 1])
    with pytest.raises(ValueError, match="seeds per type"):
        sample_subgraphs_device(dg, None, 1, 4, [a, {"author": [[1, 0], [2, 0]]}], [0, 1])       # the same count, of another type
    with pytest.raises(ValueError):
        sample_subgraphs_device(dg, None, 1, 4, [], [])      # B = 0
    with pytest.raises(ValueError):
        sample_subgraphs_device(dg, None, 1, 4, [a] * (_lib.HGT_SAMPLER_MAX_BATCH + 1), range(_lib.HGT_SAMPLER_MAX_BATCH + 1))
    with pytest.raises(ValueError):
        sample_subgraphs_device(dg, None, 1, _lib.HGT_SAMPLER_MAX_NUMBER + 1, [a], [0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sample_subgraphs_device(dg, None, 1, 4, [a, a], [0, 1])
    assert sample_subgraphs_host(dg, None, 1, 4, [], []) == []
