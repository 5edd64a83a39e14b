"""The device sampler on the GPU (csrc/hgt_sampler.hip through pyhgt_amd/sampler.py): every kernel fed the device's own state and
compared with the numpy rule, then whole calls against the fixtures, the host sibling and the invariants of a sampled sub-graph,
and the result through GNN / stack_device_graphs against the same arrays handed over by to_device_graph.

The `lines` graph (3 types, 5 meta triples, ~10^4 nodes: one row must be longer than the 8192 Philox words a hub workgroup keeps in
registers) has rows on both sides of every line of the kernels: degrees sampled_number - 1 / = / + 1 for sampled_number 8 and 128, a
row of 512 neighbours (the last a wavefront takes) and of 513 (the first a workgroup takes), one of 9000."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import test_sampler as TS
from pyhgt_amd import GNN, GraphPlan
from pyhgt_amd.sampled import SchemaGraph, stack_device_graphs, to_device_graph
from pyhgt_amd.sampler import (DeviceHeteroGraph, DeviceSamplerState, sample_subgraph_device, sample_subgraph_host, np_apply_budget,
                               np_budget_contributions, np_induce, np_select_keys, _stamp_time, TIME_NONE)
from test_hgt_gpu import DEV

pytestmark = pytest.mark.gpu

G = TS.G
TYPES = ["x", "y", "z"]
META = [("x", "y", "xy"), ("y", "x", "rev_xy"), ("x", "x", "xx"), ("x", "z", "xz"), ("z", "x", "rev_xz")]
N = {"x": 400, "y": 10000, "z": 50}
ROW_DEG = {0: 7, 1: 8, 2: 9, 3: 512, 4: 513, 5: 127, 6: 128, 7: 129, 8: 9000, 9: 0}      # degree of x_i in (x, y, xy)
MARGIN = 1.0 + 2.0 ** -20      # 16 fp32 ulps: logf / log1pf at <= 2 ulp, a multiply and a divide


def _lines_csr():
    rng = np.random.default_rng(12)
    deg = rng.poisson(3, N["x"])
    deg[10:40] = 200                                                          # 30 rows of 200: ~3000 distinct candidates at k = 128
    for i, d in ROW_DEG.items():
        deg[i] = d
    tgt = np.repeat(np.arange(N["x"]), deg)
    src = np.concatenate([rng.choice(N["y"], size=d, replace=False) for d in deg])
    tm = rng.integers(1990, 2011, size=src.size)
    tm[rng.random(src.size) < 0.1] = TIME_NONE
    xx_t = np.repeat(np.arange(N["x"]), 2)
    xx_s = (xx_t * 7 + np.tile([1, 3], N["x"])) % N["x"]
    xz_t, xz_s = np.arange(N["x"]), np.arange(N["x"]) % N["z"]
    coo = [(tgt, src, tm), (src, tgt, tm), (xx_t, xx_s, rng.integers(1990, 2011, size=xx_t.size)), (xz_t, xz_s, np.full(N["x"], TIME_NONE)),
           (xz_s, xz_t, rng.integers(1990, 2011, size=N["x"]))]
    csr = []
    for (tt, _, _), (t, s, m) in zip(META, coo):
        order = np.argsort(t, kind="stable")
        indptr = np.concatenate([[0], np.cumsum(np.bincount(t, minlength=N[tt]))])
        csr.append((indptr, s[order], m[order]))
    return csr


@pytest.fixture(scope="module")
def lines():
    rng = np.random.default_rng(13)
    feats = {t: rng.standard_normal((N[t], 24)).astype(np.float32) for t in TYPES}
    return DeviceHeteroGraph.from_csr(TYPES, META, N, _lines_csr(), feats, device=DEV)


@pytest.fixture(scope="module")
def small_dev():
    feats = {t: np.arange(G.N_NODES[t], dtype=np.float32).reshape(-1, 1) for t in G.TYPES}
    return DeviceHeteroGraph.from_csr(G.TYPES, G.META, G.N_NODES, G.csr_from_edges(G.synthetic_edges()), feats, device=DEV)


def _seeded(dg, n_seed, depth, sn):
    """a clean state with x_0 .. x_{n_seed - 1} as seeds (time 2005)"""
    st = DeviceSamplerState(dg, [n_seed, 0, 0], depth, sn)
    st.clear()
    st.seed_nodes(0, np.arange(n_seed), np.full(n_seed, 2005), 0)
    return st


def _np_budget(dg, snap, t, new, step, sn, max_time, seed):
    """the numpy rule applied to a snapshot of the device state, in place; -> first touches per type"""
    fresh = [np.zeros(0, np.int64) for _ in dg.types]
    times = _stamp_time(snap["stamp"][t][new])
    for m, (tt, st, _) in enumerate(dg.tri_types):
        if tt == t:
            s, add, stamps = np_budget_contributions(dg.csr[m], m, new, times, step, sn, max_time, seed, snap["serial"][st])
            fresh[st] = np.concatenate([fresh[st], np_apply_budget(snap["score"][st], snap["stamp"][st], s, add, stamps)])
    return fresh


@pytest.mark.parametrize("sn", [8, 128])
def test_add_budget_scores_and_stamps_exactly(lines, sn):
    n_seed, max_time, seed = 40, 2008, 77
    st = _seeded(lines, n_seed, 1, sn)
    try:
        want = st.snapshot()
        st.add_budget(0, 0, n_seed, max_time, seed)
        got = st.snapshot()
        fresh = _np_budget(lines, want, 0, np.arange(n_seed), 0, sn, max_time, seed)
        for t in range(3):
            assert np.array_equal(got["score"][t], want["score"][t]), "score of %s" % TYPES[t]
            assert np.array_equal(got["stamp"][t], want["stamp"][t]), "stamp of %s" % TYPES[t]
            assert np.array_equal(np.sort(got["cand"][t]), fresh[t]) and got["counts"][t, 3] == 0
        assert len(got["cand"][1]) > (2500 if sn == 128 else 64)
        # a second step of the same type adds on top (an inherited time, a later step's stamp): select x, then its budget
        st.select(0, 3, seed)
        want = st.snapshot()
        new = want["sampled"][0][n_seed:]
        assert len(new) == min(sn, len(got["cand"][0]))
        st.add_budget(0, 3, sn, max_time, seed)
        got = st.snapshot()
        _np_budget(lines, want, 0, new, 3, sn, max_time, seed)
        for t in range(3):
            assert np.array_equal(got["score"][t], want["score"][t]) and np.array_equal(got["stamp"][t], want["stamp"][t])
    finally:
        st.clear()


def _check_select(st, dg, t, step, seed, sn):
    before = st.snapshot()
    st.select(t, step, seed)
    after = st.snapshot()
    cand, base = before["cand"][t], len(before["sampled"][t])
    count = min(sn, len(cand))
    chosen = after["sampled"][t][base:]
    assert len(chosen) == count and after["counts"][t, 1] == base and after["counts"][t, 0] == base + count
    assert set(chosen.tolist()) <= set(cand.tolist()) and len(set(chosen.tolist())) == count
    assert np.array_equal(np.sort(after["cand"][t]), np.setdiff1d(cand, chosen))
    assert np.array_equal(after["serial"][t][chosen], np.arange(base, base + count))
    assert np.array_equal(after["score"][t], before["score"][t]) and np.array_equal(after["stamp"][t], before["stamp"][t])
    keys = dict(zip(cand.tolist(), np_select_keys(cand, before["score"][t], t, step, seed)))
    k_chosen = np.array([keys[v] for v in chosen.tolist()])
    rest = np.array([keys[v] for v in np.setdiff1d(cand, chosen).tolist()])
    ratio = 0.0
    if count and rest.size:
        ratio = k_chosen.max() / rest.min()
        assert ratio <= MARGIN, "a chosen key is %.9g x the smallest key left behind" % ratio
    order = 0.0
    if count > 1:
        order = (k_chosen[:-1] / k_chosen[1:]).max()
        assert order <= MARGIN, "serial order: a key is %.9g x its successor" % order
    print("select %s: %d of %d candidates, largest chosen / smallest left = %.9f, largest key / successor = %.9f"
          % (TYPES[t], count, len(cand), ratio, order))
    return count, len(cand)


@pytest.mark.parametrize("n_seed", [7, 8, 9])
def test_select_at_k_minus_one_k_and_k_plus_one_candidates(lines, n_seed):
    """x_i -> z_(i % 50): n_seed seeds leave exactly n_seed candidates of z, a list shorter than a wavefront, at k = 8"""
    st = _seeded(lines, n_seed, 1, 8)
    try:
        st.add_budget(0, 0, n_seed, None, 5)
        assert _check_select(st, lines, 2, 5, 5, 8) == (min(8, n_seed), n_seed)
    finally:
        st.clear()


def test_select_from_a_list_that_spans_several_workgroups(lines):
    st = _seeded(lines, 40, 3, 128)
    try:
        st.add_budget(0, 0, 40, 2008, 6)
        count, n = _check_select(st, lines, 1, 4, 6, 128)
        assert count == 128 and 2500 < n < 4500
        _check_select(st, lines, 1, 7, 6, 128)                # once more on what was left
        _check_select(st, lines, 0, 6, 6, 128)
    finally:
        st.clear()


@pytest.mark.parametrize("sn", [8, 128])
def test_induce_equals_the_numpy_induction_of_the_devices_node_set(lines, sn):
    st = _seeded(lines, 12, 2, sn)                            # seeds x_0 .. x_11: the rows of 512, 513 and 9000 neighbours among them
    try:
        st.add_budget(0, 0, 12, 2008, 9)
        for layer in range(2):
            for t in range(3):
                st.select(t, 3 * (1 + layer) + t, 9)
                st.add_budget(t, 3 * (1 + layer) + t, sn, 2008, 9)
        snap = st.snapshot()
        src, dst, etime, rel_ptr, type_off, node_time, node_id, n_per_type = st.induce()
        times = [_stamp_time(snap["stamp"][t][snap["sampled"][t]]) for t in range(3)]
        want = np_induce(lines, snap["sampled"], times, snap["serial"])
        for got, exp, name in zip((src, dst, etime, rel_ptr, type_off), want, ("src", "dst", "edge_time", "rel_ptr", "type_off")):
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), exp), name
        assert n_per_type == [len(s) for s in snap["sampled"]] and n_per_type[1] == 2 * sn
        assert np.array_equal(node_id.cpu().numpy(), np.concatenate(snap["sampled"]))
        assert np.array_equal(node_time.cpu().numpy(), np.concatenate(times))
        assert int(rel_ptr[1] - rel_ptr[0]) > 0 and int(rel_ptr[2] - rel_ptr[1]) > 0
        st.reset()
        clean = st.snapshot()
        for t in range(3):
            assert not clean["score"][t].any() and not clean["stamp"][t].any() and (clean["serial"][t] == -1).all()
        assert not clean["counts"].any()
    finally:
        st.clear()


# ---------------------------------------------------------------------------------------------------------------- whole calls
def _canonical(res):
    cpu = lambda v: v.cpu().numpy()
    return G.canonical(list(res[5]), {t: cpu(v) for t, v in res.indxs.items()}, {t: cpu(v) for t, v in res.times.items()}, cpu(res[3]),
                       cpu(res[4]), cpu(res[2]), res[5])


@pytest.mark.parametrize("case", list(G.CASES))
def test_deterministic_regime_equals_fixtures_and_host(small_dev, case):
    fx = np.load(G.GOLDEN)
    inp, max_time, depth = G.CASES[case]
    res = sample_subgraph_device(small_dev, max_time, depth, G.SAMPLED_NUMBER, inp, seed=3)
    host = sample_subgraph_host(small_dev, max_time, depth, G.SAMPLED_NUMBER, inp, seed=3)
    nodes, rows = _canonical(res)
    nodes_h, rows_h = TS._canonical(host)
    for t in G.TYPES:
        assert np.array_equal(nodes[t], fx["%s/nodes/%s" % (case, t)]) and np.array_equal(nodes[t], nodes_h[t]), t
    assert np.array_equal(rows, fx["%s/edges" % case]) and np.array_equal(rows, rows_h)
    assert res[5] == host[5] and res[6] == host[6]
    assert torch.equal(res[0].cpu()[:, 0], torch.cat([res.indxs[t] for t in G.TYPES]).cpu().float())
    res.plan.raise_if_bad(wait=True)


def test_random_regime_is_valid_and_repeatable(lines):
    inp = {"x": [[i, 2005] for i in range(12)], "z": [[3, 2001]]}
    sn, depth = 16, 3
    a = sample_subgraph_device(lines, 2008, depth, sn, inp, seed=31)
    b = sample_subgraph_device(lines, 2008, depth, sn, inp, seed=31)
    c = sample_subgraph_device(lines, 2008, depth, sn, inp, seed=32)
    for u, v in zip(list(a[:5]) + list(a.sorted), list(b[:5]) + list(b.sorted)):
        assert torch.equal(u, v)                              # the same seed gives the same bits twice
    assert any(not torch.equal(a.indxs[t], c.indxs[t]) for t in TYPES if a.indxs[t].shape == c.indxs[t].shape) or \
        any(a.indxs[t].shape != c.indxs[t].shape for t in TYPES)
    ids = [a.indxs[t].cpu().numpy() for t in TYPES]
    # per-step counts: y and x always have more than sn candidates; z has 50 nodes in all
    assert len(ids[0]) == 12 + depth * sn and len(ids[1]) == depth * sn and 1 <= len(ids[2]) <= 1 + depth * sn
    assert ids[0][:12].tolist() == list(range(12)) and ids[2][0] == 3
    serial = []
    for t in range(3):                                        # the serials are a permutation: distinct ids inside the type
        assert len(set(ids[t].tolist())) == len(ids[t]) and ids[t].min() >= 0 and ids[t].max() < N[TYPES[t]]
        s = np.full(N[TYPES[t]], -1, np.int32)
        s[ids[t]] = np.arange(len(ids[t]))
        serial.append(s)
    # every edge exists in the graph and no edge between sampled nodes is missing: the numpy induction of this node set, exactly
    times = [a.times[t].cpu().numpy() for t in TYPES]
    for got, exp in zip(a.sorted, np_induce(lines, ids, times, serial)):
        assert np.array_equal(got.cpu().numpy(), exp)
    assert (times[0][12:] <= 2008).all() and (times[1] <= 2008).all()
    assert torch.equal(a[0], torch.cat([lines.features[t][a.indxs[TYPES[t]]] for t in range(3)]))
    a.plan.raise_if_bad(wait=True)
    # the host sibling draws the same words: the same node sets unless an fp32 key order differs from the float64 one
    h = sample_subgraph_host(lines, 2008, depth, sn, inp, seed=31)
    same = [np.array_equal(np.sort(h.indxs[t]), np.sort(ids[i])) for i, t in enumerate(TYPES)]
    print("node sets equal to the host sibling's:", same)


def _hand_over(res, dg):
    """the arrays of a sampled graph as (feature, time, edge_list, graph): what to_device_graph takes"""
    types = dg.get_types()
    src, dst, _, rel_ptr, type_off = [v.cpu().numpy() for v in res.sorted]
    feat, off = res[0].cpu().numpy(), type_off
    feature = {t: feat[off[i]:off[i + 1]] for i, t in enumerate(types)}
    time = {t: res.times[t].cpu().numpy() for t in types}
    edge_list = OrderedDict()
    for t in types:
        if len(feature[t]):
            edge_list.setdefault(t, OrderedDict()).setdefault(t, OrderedDict())["self"] = [[i, i] for i in range(len(feature[t]))]
    tid = {t: i for i, t in enumerate(types)}
    for (tt, st, rel) in dg.triples:
        r = dg.edge_dict[rel]
        e = slice(rel_ptr[r], rel_ptr[r + 1])
        pairs = np.stack([dst[e] - off[tid[tt]], src[e] - off[tid[st]]], axis=1)
        if len(pairs):
            edge_list.setdefault(tt, OrderedDict()).setdefault(st, OrderedDict())[rel] = pairs
    return feature, time, edge_list, SchemaGraph(types, dg.get_meta_graph())


def test_sampled_graph_runs_through_gnn_and_stacking_like_a_handed_over_one(lines):
    GraphPlan.clear_cache()
    inp = {"x": [[i, 2005] for i in range(16)]}
    parts = [sample_subgraph_device(lines, 2008, 2, 24, inp, seed=s, plan=(s == 41)) for s in (41, 42)]
    twins = [to_device_graph(*_hand_over(p, lines), device=DEV, plan=(i == 0)) for i, p in enumerate(parts)]
    for p, q in zip(parts, twins):
        for i in range(5):
            assert p[i].dtype == q[i].dtype and torch.equal(p[i], q[i]), i
        assert p[5] == q[5] and p[6] == q[6] and p[3].stride() == q[3].stride()
        assert all(torch.equal(u, v) for u, v in zip(p.sorted, q.sorted))
    T, R = len(TYPES), len(lines.edge_dict)
    assert GraphPlan.cached(parts[0][1], parts[0][3], parts[0][4], parts[0][2], T, R) is parts[0].plan
    torch.manual_seed(4)
    gnn = GNN(24, 64, T, R, 4, 2, prev_norm=True, last_norm=True, use_RTE=True).eval().to(DEV)
    S, D = stack_device_graphs(parts), stack_device_graphs(twins)
    with torch.no_grad():
        out = gnn(*parts[0][:5])
        twin = gnn(*twins[0][:5])
        out_s, twin_s = gnn(*S[:5]), gnn(*D[:5])
    assert torch.isfinite(out).all() and torch.equal(out, twin)
    assert torch.equal(out_s, twin_s) and out_s.shape[0] == parts[0][1].numel() + parts[1][1].numel()
    S.plan.raise_if_bad(wait=True)
    GraphPlan.clear_cache()
