"""The batched device sampler on the GPU: one sample_subgraphs_device call against the host rule and against the single device calls,
bit for bit -- replicas with identical seed nodes (any state shared between replicas would change a result), replicas of different
sizes (the fill offsets), an empty replica, hub queues in two replicas at once, the kernel-argument tables at their limits, masks, the
step-level calls against the numpy rule per replica, the state rule after a call that raised, the hand-over to stack_device_graphs
and GNN, and the number of launches, which does not depend on B.  Graphs and certified calls are those of test_sampler.py /
test_sampler_gpu.py."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import test_sampler as TS
import test_sampler_gpu as TG
from pyhgt_amd import GNN, GraphPlan, _lib, sample_subgraphs_device, seed_edge_mask
from pyhgt_amd.sampled import stack_device_graphs
from pyhgt_amd.sampler import (BatchedDeviceSamplerState, _batched_state, _stamp_time, np_induce, sample_subgraph_device,
                               sample_subgraph_host)
from test_hgt_gpu import DEV

pytestmark = pytest.mark.gpu

lines, oag_dev = TG.lines, TG.oag_dev
MAXB = _lib.HGT_SAMPLER_MAX_BATCH


def _groups(calls):
    """calls that share (seeds, max_time, depth, sampled_number) and differ in the Philox seed"""
    out = OrderedDict()
    for c in calls:
        out.setdefault((id(c[0]),) + c[1:4], []).append(c)
    return list(out.values())


OAG_GROUPS = _groups(TS.OAG_CALLS)


def _batched(dg, calls, plan=False, mask=None):
    inp, max_time, depth, sn = calls[0][:4]
    assert all(c[1:4] == calls[0][1:4] for c in calls)
    return sample_subgraphs_device(dg, max_time, depth, sn, [c[0] for c in calls], [c[4] for c in calls], plan=plan, mask=mask)


def _single(dg, call, plan=False, mask=None):
    inp, max_time, depth, sn, seed = call
    return sample_subgraph_device(dg, max_time, depth, sn, inp, seed, plan=plan, mask=mask)


def _assert_same(a, b):
    TG._assert_same(a, b)
    assert a.n_seed == b.n_seed and all(torch.equal(a.seed_rows(t), b.seed_rows(t)) for t in a.n_seed)
    assert all(u.dtype == v.dtype and u.shape == v.shape and u.stride() == v.stride() for u, v in zip(a[:5], b[:5]))


# ---------------------------------------------------------------------------------------------------------------- 1. the host rule
def test_the_groups_are_what_the_checks_need():
    sizes = sorted(len(g) for g in OAG_GROUPS)
    assert sum(1 for s in sizes if s >= 2) >= 6 and sizes[-1] == 4 and sum(sizes) == len(TS.OAG_CALLS)


@pytest.mark.parametrize("i", range(len(OAG_GROUPS)))
def test_group_of_certified_calls_equals_the_host_rule(oag_dev, i):
    """the replicas of a group have identical seed nodes and differ only in the Philox seed"""
    group = OAG_GROUPS[i]
    hosts = [TG._certified_host(oag_dev, c) for c in group]
    got = _batched(oag_dev, group)
    assert len(got) == len(group)
    for res, host in zip(got, hosts):
        TG._assert_equals_host(res, host, oag_dev)
        assert res.plan is None and res.n_seed == host.n_seed
    if len(group) > 1 and group[0][2] > 0:
        assert any(not np.array_equal(hosts[0].sorted[0], h.sorted[0]) for h in hosts[1:])


# ---------------------------------------------------------------------------------------------------------------- 2. the single call
def _window(b, n=12):
    """replica 0 owns the rows of 512, 513 and 9000 neighbours, the others own none"""
    lo = 0 if b == 0 else 90 + 4 * b
    return {"x": [[i, 2005] for i in range(lo, lo + n)]}


@pytest.mark.parametrize("max_time", [2008, None])
@pytest.mark.parametrize("sn", [8, 128])
@pytest.mark.parametrize("B", [1, 2, MAXB])
def test_each_replica_equals_its_single_call(lines, B, sn, max_time):
    calls = [(_window(b), max_time, 2, sn, 1000 + b) for b in range(B)]
    got = _batched(lines, calls)
    want = [_single(lines, c) for c in calls]
    for res, one in zip(got, want):
        _assert_same(res, one)
    assert torch.equal(got[0][0], torch.cat([lines.features[t][got[0].indxs[TG.TYPES[t]]] for t in range(3)]))
    shapes = {(int(r[1].numel()), int(r[4].numel())) for r in got}
    assert B == 1 or len(shapes) > 1, "the replicas have the same node and edge counts: the fill offsets are not exercised"
    assert len(got[0].indxs["y"]) == 2 * sn


def test_twin_replicas_are_equal(lines):
    calls = [(_window(0), 2008, 2, 8, 5), (_window(3), 2008, 2, 8, 6), (_window(0), 2008, 2, 8, 5)]
    got = _batched(lines, calls)
    _assert_same(got[0], got[2])
    assert not torch.equal(got[0].indxs["x"], got[1].indxs["x"])


# ---------------------------------------------------------------------------------------------------------------- 3. an empty replica
@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_replica_without_in_neighbours(where):
    """x_30 .. x_39 have no neighbour in either direction: the piece of a replica seeded there is its seeds and their `self` edges"""
    sn = 4
    dg = TG._rows_graph(40, 60, [10] * 30 + [0] * 10, 31)
    full = [({"x": [[i, 2005] for i in range(4 * k, 4 * k + 4)]}, 2008, 2, sn, 40 + k) for k in range(2)]
    empty = ({"x": [[i, 2005] for i in range(30, 34)]}, 2008, 2, sn, 50)
    calls = full[:where] + [empty] + full[where:]
    got = _batched(dg, calls)
    for res, call in zip(got, calls):
        _assert_same(res, _single(dg, call))
    e = got[where]
    assert e.indxs["x"].tolist() == [30, 31, 32, 33] and e.indxs["y"].numel() == 0
    assert e.sorted[3].tolist() == [0, 0, 0, 4] and e.sorted[0].tolist() == e.sorted[1].tolist() == [0, 1, 2, 3]
    for k, res in enumerate(got):
        if k != where:
            assert res.indxs["y"].numel() == 2 * sn and res.indxs["x"].numel() == 4 + sn      # x has no candidate before y's first budget


# ---------------------------------------------------------------------------------------------------------------- 4. hub queues
def _assert_budget(st, dg, t, new, step, sn, max_time, seeds):
    """one batched add_budget against the numpy rule applied to every replica's own snapshot; new[b]: the newest batch of replica b"""
    want = st.snapshot()
    st.add_budget(t, step, max(len(v) for v in new), max_time, seeds)
    got = st.snapshot()
    for b in range(st.B):
        fresh = TG._np_budget(dg, want[b], t, np.asarray(new[b], dtype=np.int64), step, sn, max_time, seeds[b])
        for i, name in enumerate(dg.types):
            assert np.array_equal(got[b]["score"][i], want[b]["score"][i]), "score of %s, replica %d" % (name, b)
            assert np.array_equal(got[b]["stamp"][i], want[b]["stamp"][i]), "stamp of %s, replica %d" % (name, b)
            assert np.array_equal(np.sort(got[b]["cand"][i]), np.union1d(want[b]["cand"][i], fresh[i])) and got[b]["counts"][i, 3] == 0
    return got


def _assert_induce(st, dg):
    snap = st.snapshot()
    src, dst, etime, rel_ptr, type_off, node_time, node_id, n_per_type, node_off, edge_off = st.induce()
    for b in range(st.B):
        n, e = slice(node_off[b], node_off[b + 1]), slice(edge_off[b], edge_off[b + 1])
        times = [_stamp_time(snap[b]["stamp"][t][snap[b]["sampled"][t]]) for t in range(len(dg.types))]
        want = np_induce(dg, snap[b]["sampled"], times, snap[b]["serial"])
        for got, exp, name in zip((src[e], dst[e], etime[e], rel_ptr[b], type_off[b]), want, ("src", "dst", "edge_time", "rel_ptr", "type_off")):
            assert np.array_equal(got.cpu().numpy(), exp), "%s of replica %d" % (name, b)
        assert n_per_type[b] == [len(v) for v in snap[b]["sampled"]]
        assert np.array_equal(node_id[n].cpu().numpy(), np.concatenate(snap[b]["sampled"]))
        assert np.array_equal(node_time[n].cpu().numpy(), np.concatenate(times))
    return rel_ptr.cpu().numpy()


def _assert_clean(st):
    for snap in st.snapshot():
        assert not any(a.any() for a in snap["score"] + snap["stamp"]) and all((a == -1).all() for a in snap["serial"])
        assert not snap["counts"].any()


def test_more_hub_rows_than_hub_workgroups_in_two_replicas():
    """the graph of test_more_hub_rows_than_hub_workgroups: both replicas queue 300 rows for 256 hub workgroups, each in its own queue"""
    n_seed, sn, max_time, seeds = 300, 16, 2008, [21, 22]
    dg = TG._rows_graph(304, 2000, np.random.default_rng(20).integers(513, 601, size=304), 22)
    st = BatchedDeviceSamplerState(dg, [n_seed, 0], 1, sn, 2)
    st.clear()
    try:
        ids = np.stack([np.arange(n_seed), np.arange(4, 4 + n_seed)])
        st.seed_nodes(0, ids, np.full_like(ids, 2005), 0)
        _assert_budget(st, dg, 0, ids, 0, sn, max_time, seeds)
        assert st.hub[:2].tolist() == [n_seed, n_seed] and n_seed > TG._hub_blocks()
        n_x = [n_seed, n_seed]
        for t in (1, 0):
            st.select(t, 2 + t, seeds)
            snap = st.snapshot()
            new = [s["sampled"][t][s["counts"][t, 1]:] for s in snap]
            assert all(len(v) == sn for v in new) if t else all(1 <= len(v) <= 4 for v in new)
            _assert_budget(st, dg, t, new, 2 + t, sn, max_time, seeds)
            if t == 0:
                n_x = [n_seed + len(v) for v in new]
        rel_ptr = _assert_induce(st, dg)
        assert st.hub[:2].tolist() == n_x and min(n_x) > TG._hub_blocks() and (rel_ptr[:, 1] > 0).all() and (rel_ptr[:, 2] > rel_ptr[:, 1]).all()
        st.reset()
        _assert_clean(st)
    finally:
        st.clear()


# ---------------------------------------------------------------------------------------------------------------- 5. tables
@pytest.mark.parametrize("kind, i", [("wide", 0), ("wide", 1), ("one", 0), ("one", 1)])
def test_tables_at_their_limits(kind, i):
    dg = TS.table_graph(kind, device=DEV)
    call = TS.TABLE_CALLS[kind][i]
    host = TG._certified_host(dg, call)
    for res in _batched(dg, [call, call]):
        TG._assert_equals_host(res, host, dg)


# ---------------------------------------------------------------------------------------------------------------- 6. masks
def test_masked_batched_call(oag_dev):
    group = next(g for g in OAG_GROUPS if len(g) == 4)
    inp, max_time, depth, sn = group[0][:4]
    assert inp is TS._PAPERS and depth == 3
    mask = seed_edge_mask(oag_dev, ["PV", "rev_PV"], "paper", len(inp["paper"]))
    got = _batched(oag_dev, group, mask=mask)
    plain = _batched(oag_dev, group)
    for res, raw, call in zip(got, plain, group):
        TG._certified_host(oag_dev, call)                     # the mask enters the induction only: the certificate is the plain call's
        _assert_same(res, _single(oag_dev, call, mask=mask))
        TG._assert_equals_host(res, sample_subgraph_host(oag_dev, max_time, depth, sn, inp, call[4], mask=mask), oag_dev)
        assert res[4].numel() < raw[4].numel()
    zero = {tri: (0, 0) for tri in mask}
    for res, raw in zip(_batched(oag_dev, group, mask=zero), plain):
        _assert_same(res, raw)


# ---------------------------------------------------------------------------------------------------------------- 7. step level
def test_step_level_calls_per_replica(lines):
    sn, seeds, n = 8, [7, 8, 9], 12
    st = BatchedDeviceSamplerState(lines, [n, 0, 0], 1, sn, 3)
    st.clear()
    try:
        ids = np.stack([np.arange(lo, lo + n) for lo in (0, 5, 200)])
        st.seed_nodes(0, ids, np.full_like(ids, 2005), 0)
        snap = st.snapshot()
        assert len(snap) == 3 and all(np.array_equal(s["sampled"][0], ids[b]) for b, s in enumerate(snap))
        got = _assert_budget(st, lines, 0, ids, 0, sn, 2008, seeds)
        assert len({len(s["cand"][1]) for s in got}) > 1
        st.reset()
        assert not st.dirty
        _assert_clean(st)
    finally:
        st.clear()


# ---------------------------------------------------------------------------------------------------------------- 8. the state rule
def _fail_on_features(dg, calls):
    i = dg.types.index("author")
    keep, dg.features[i] = dg.features[i], None
    try:
        with pytest.raises(ValueError, match="no feature matrix"):
            _batched(dg, calls)
    finally:
        dg.features[i] = keep


def _fail_on_overflow(dg, calls):
    st = _batched_state(dg, [len(calls[0][0].get(t, [])) for t in dg.types], calls[0][2], calls[0][3], len(calls))
    i = dg.types.index("author")
    keep, st.types_c[i].cap_cand = st.types_c[i].cap_cand, 5
    try:
        with pytest.raises(RuntimeError, match="overflowed"):
            _batched(dg, calls)
    finally:
        st.types_c[i].cap_cand = keep


@pytest.mark.parametrize("fail", [_fail_on_features, _fail_on_overflow], ids=["ValueError", "RuntimeError"])
def test_a_failed_batched_call_does_not_poison_the_next(oag_dev, fail):
    a = next(g for g in OAG_GROUPS if len(g) == 4)            # _PAPERS, depth 3, 16
    b = next(g for g in OAG_GROUPS if g[0][0] is TS._THREE and g[0][2:4] == (3, 128))
    fail(oag_dev, a[:3])
    assert oag_dev._batch_dirty
    one = _single(oag_dev, a[0])                              # a single call in between: its own arrays, its own flag
    TG._assert_equals_host(one, TG._certified_host(oag_dev, a[0]), oag_dev)
    assert oag_dev._batch_dirty and not oag_dev._dev_dirty
    for res, call in zip(_batched(oag_dev, b), b):            # another B, another shape
        TG._assert_equals_host(res, TG._certified_host(oag_dev, call), oag_dev)
        _assert_same(res, _single(oag_dev, call))
    assert not oag_dev._batch_dirty
    for res, call in zip(_batched(oag_dev, a), a):            # and the shape that failed, at another B
        TG._assert_equals_host(res, TG._certified_host(oag_dev, call), oag_dev)


# ---------------------------------------------------------------------------------------------------------------- 9. hand-over
def test_pieces_stack_and_run_like_single_calls(lines):
    GraphPlan.clear_cache()
    calls = [(_window(b, 16), 2008, 2, 24, 41 + b) for b in range(3)]
    S = stack_device_graphs(_batched(lines, calls))
    D = stack_device_graphs([_single(lines, c) for c in calls])
    assert all(torch.equal(u, v) for u, v in zip(list(S[:5]) + list(S.sorted), list(D[:5]) + list(D.sorted))) and S[5] == D[5]
    piece, one = _batched(lines, calls, plan=True)[1], _single(lines, calls[1], plan=True)
    T, R = len(TG.TYPES), len(lines.edge_dict)
    assert piece.plan is not None and GraphPlan.cached(piece[1], piece[3], piece[4], piece[2], T, R) is piece.plan
    torch.manual_seed(4)
    gnn = GNN(24, 64, T, R, 4, 2, prev_norm=True, last_norm=True, use_RTE=True).eval().to(DEV)
    with torch.no_grad():
        out, twin = gnn(*piece[:5]), gnn(*one[:5])
    assert torch.isfinite(out).all() and torch.equal(out, twin)
    piece.plan.raise_if_bad(wait=True)
    GraphPlan.clear_cache()


# ---------------------------------------------------------------------------------------------------------------- 10. launches
class _Counting:
    """the loaded library with the calls of the sampler entry points written down"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("hgt_sampler_"):
            return fn

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


def test_the_number_of_sampler_calls_does_not_depend_on_b(lines):
    seen = {}
    for B in (1, 8):
        calls = [(_window(b), 2008, 2, 8, 70 + b) for b in range(B)]
        st = _batched_state(lines, [12, 0, 0], 2, 8, B)
        lib, st.lib = st.lib, _Counting(st.lib)
        try:
            _batched(lines, calls)
            seen[B] = st.lib.calls
        finally:
            st.lib = lib
    assert seen[1] == seen[8] and len(seen[1]) > 10
    assert seen[1].count("hgt_sampler_gather_features") == 1 and all(n.endswith("_batched") or n == "hgt_sampler_gather_features" for n in seen[1])
