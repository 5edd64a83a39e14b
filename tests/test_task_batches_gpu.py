"""Task batches on the GPU: the masked induction kernels (csrc/hgt_sampler.hip) against `np_induce` with the same mask on the device's
own node set, whole masked calls against the certified host sibling, a masked result through GNN / stack_device_graphs against the
same lists masked on the host and handed over, and the label kernel (csrc/hgt_sampler_labels.hip) against the numpy siblings, bit for
bit.  The calls, masks and label cases are those test_task_batches.py checks on the CPU against the reference's scripts."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import test_sampler as TS
import test_sampler_gpu as TG
import test_task_batches as TB
from pyhgt_amd import GNN, GraphPlan, LabelSpace, np_label_counts, np_label_distribution, np_label_index
from pyhgt_amd.sampled import stack_device_graphs, to_device_graph
from pyhgt_amd.sampler import DeviceHeteroGraph, sample_subgraph_device, np_induce, _device_state, _stamp_time
from test_hgt_gpu import DEV

pytestmark = pytest.mark.gpu

lines = TG.lines
oag_dev = TG.oag_dev

XY, REV_XY, XX = ("x", "y", "xy"), ("y", "x", "rev_xy"), ("x", "x", "xx")
# 12 seeds x_0 .. x_11; x_3 has 512 neighbours (the last row a wavefront takes), x_4 has 513 (the first a workgroup takes)
STEP_MASKS = OrderedDict([
    ("zero", {XY: (0, 0), REV_XY: (0, 0), XX: (0, 0)}),
    ("xy_targets_below_4", {XY: (4, 0)}),
    ("rev_xy_sources_below_12", {REV_XY: (0, 12)}),
    ("xx_both", {XX: (5, 9)}),
    ("xy_everything", {XY: (10 ** 6, 0)}),
    ("rev_xy_everything", {REV_XY: (0, 2 ** 31 - 1)}),
    ("task", {XY: (12, 0), REV_XY: (0, 12), XX: (12, 12)}),
])


@pytest.mark.parametrize("sn", [8, 128])
def test_masked_induce_equals_the_numpy_induction_of_the_devices_node_set(lines, sn):
    st = TG._seeded(lines, 12, 2, sn)
    try:
        st.add_budget(0, 0, 12, 2008, 9)
        for layer in range(2):
            for t in range(3):
                st.select(t, 3 * (1 + layer) + t, 9)
                st.add_budget(t, 3 * (1 + layer) + t, sn, 2008, 9)
        snap = st.snapshot()
        times = [_stamp_time(snap["stamp"][t][snap["sampled"][t]]) for t in range(3)]
        plain = [v.cpu().numpy() if torch.is_tensor(v) else v for v in st.induce()]
        T, M = 3, len(lines.triples)
        for name, mask in STEP_MASKS.items():
            src, dst, etime, rel_ptr, type_off, node_time, node_id, n_per_type = st.induce(mask)
            want = np_induce(lines, snap["sampled"], times, snap["serial"], mask)
            for got, exp, what in zip((src, dst, etime, rel_ptr, type_off), want, ("src", "dst", "edge_time", "rel_ptr", "type_off")):
                assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), exp), (name, what)
            rel_ptr, sizes = rel_ptr.cpu().numpy(), st.sizes.cpu().numpy()
            N = sum(n_per_type)
            assert rel_ptr[0] == 0 and rel_ptr[-1] == src.numel() and rel_ptr[-1] - rel_ptr[-2] == N and int(type_off[-1]) == N
            assert n_per_type == [len(s) for s in snap["sampled"]] == sizes[:T].tolist() and sizes[T + M] == 0
            per_triple = [int(rel_ptr[r + 1] - rel_ptr[r]) for _, _, r in lines.tri_types]     # one triple per relation in this graph
            assert sizes[T:T + M].tolist() == per_triple and sizes[T + M + 1] == sum(per_triple) == src.numel() - N
            assert np.array_equal(node_id.cpu().numpy(), plain[6]) and np.array_equal(node_time.cpu().numpy(), plain[5])
            lost = plain[0].size - src.numel()
            print("sn %d, %s: %d of %d edges left out, per triple %r" % (sn, name, lost, plain[0].size - N, per_triple))
            if name == "zero":
                assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((src, dst, etime), plain[:3])) and lost == 0
            elif name.endswith("everything"):
                assert per_triple[lines.triples.index(next(iter(mask)))] == 0 and lost > 0
            else:
                assert lost > 0
                if name == "xy_targets_below_4":                 # rows 0-3 are gone, the rest of the relation is not
                    e = dst.cpu().numpy()[rel_ptr[0]:rel_ptr[1]]
                    assert e.size > 0 and e.min() == 4           # x_4: the row of 513 neighbours, in the hub kernel
        st.reset()
        clean = st.snapshot()
        for t in range(3):
            assert not clean["score"][t].any() and not clean["stamp"][t].any() and (clean["serial"][t] == -1).all()
        assert not clean["counts"].any()
    finally:
        st.clear()


# ---------------------------------------------------------------------------------------------------------------- whole calls
_HOST = {}


def _masked_host(dg, i):
    """the host sibling's masked result of OAG call i, computed once; the call is certified by its unmasked twin (the mask does not
    enter any selection)"""
    if i not in _HOST:
        TG._certified_host(dg, TS.OAG_CALLS[i])
        _HOST[i] = TB._host(dg, TS.OAG_CALLS[i], TB.oag_mask(dg, TS.OAG_CALLS[i]))
    return _HOST[i]


def _call(dg, call, mask):
    inp, max_time, depth, sn, seed = call
    return sample_subgraph_device(dg, max_time, depth, sn, inp, seed, plan=False, mask=mask)


@pytest.mark.parametrize("i", range(len(TS.OAG_CALLS)))
def test_masked_call_equals_the_host_sibling(oag_dev, i):
    call = TS.OAG_CALLS[i]
    res = _call(oag_dev, call, TB.oag_mask(oag_dev, call))
    TG._assert_equals_host(res, _masked_host(oag_dev, i), oag_dev)
    assert res.n_seed == {t: len(call[0].get(t, [])) for t in TS.OAG_TYPES}
    for t in call[0]:
        rows = res.seed_rows(t)
        assert rows.device == res[1].device and rows.dtype == torch.int64 and (res[1][rows] == TS.OAG_TYPES.index(t)).all()
        assert res.indxs[t][:len(call[0][t])].tolist() == [v[0] for v in call[0][t]]
    plain = _call(oag_dev, call, None)
    TG._assert_same(_call(oag_dev, call, {tri: (0, 0) for tri in oag_dev.triples}), plain)
    TG._assert_same(_call(oag_dev, call, {}), plain)


# ---------------------------------------------------------------------------------------------------------------- hand-over
def _hand_over_masked(res, dg, mask):
    """the lists of an UNMASKED device result with the rule applied on the host: what to_device_graph takes"""
    feature, time, edge_list, graph = TG._hand_over(res, dg)
    for (tt, st, rel), (tgt_below, src_below) in mask.items():
        pairs = edge_list.get(tt, {}).get(st, {}).get(rel)
        if pairs is not None:
            kept = pairs[(pairs[:, 0] >= tgt_below) & (pairs[:, 1] >= src_below)]
            if len(kept):
                edge_list[tt][st][rel] = kept
            else:
                del edge_list[tt][st][rel]
    return feature, time, edge_list, graph


def test_masked_graph_runs_through_gnn_and_stacking_like_a_handed_over_one(oag_dev):
    GraphPlan.clear_cache()
    calls = [TS.OAG_CALLS[2], TS.OAG_CALLS[7]]                  # call 2 comes out with empty relations, call 7 without
    masks = [TB.oag_mask(oag_dev, c) for c in calls]
    parts = [sample_subgraph_device(oag_dev, c[1], c[2], c[3], c[0], c[4], plan=(k == 1), mask=m) for k, (c, m) in enumerate(zip(calls, masks))]
    twins = [to_device_graph(*_hand_over_masked(_call(oag_dev, c, None), oag_dev, m), device=DEV, plan=(k == 1))
             for k, (c, m) in enumerate(zip(calls, masks))]
    R = len(oag_dev.edge_dict)
    per_rel = [np.diff(p.sorted[3].cpu().numpy()) for p in parts]
    assert (per_rel[0][:R - 1] == 0).any() and (per_rel[1][:R - 1] > 0).sum() >= 8
    for p, q in zip(parts, twins):
        for i in range(5):
            assert p[i].dtype == q[i].dtype and torch.equal(p[i], q[i]), i
        assert p[5] == q[5] and p[6] == q[6] and all(torch.equal(u, v) for u, v in zip(p.sorted, q.sorted))
    T = len(TS.OAG_TYPES)
    torch.manual_seed(4)
    gnn = GNN(8, 64, T, R, 4, 2, prev_norm=True, last_norm=True, use_RTE=True).eval().to(DEV)
    S, D = stack_device_graphs(parts), stack_device_graphs(twins)
    with torch.no_grad():
        out, twin = gnn(*parts[1][:5]), gnn(*twins[1][:5])
        out_s, twin_s = gnn(*S[:5]), gnn(*D[:5])
    assert torch.isfinite(out).all() and torch.equal(out, twin)
    assert torch.equal(out_s, twin_s) and out_s.shape[0] == parts[0][1].numel() + parts[1][1].numel()
    S.plan.raise_if_bad(wait=True)
    GraphPlan.clear_cache()


# ---------------------------------------------------------------------------------------------------------------- labels
def _assert_labels(space, host_graph, ids, t_min, t_max, ids_dev=None):
    """the three outputs of the kernel against the siblings; the distribution inside a wider matrix whose padding must survive"""
    ids_dev = ids if ids_dev is None else ids_dev
    C, n = space.n_cols, len(ids)
    want = (np_label_distribution(host_graph, space.triple, space.col_of, C, ids, t_min, t_max),
            np_label_index(host_graph, space.triple, space.col_of, ids, t_min, t_max),
            np_label_counts(host_graph, space.triple, space.col_of, ids, t_min, t_max))
    dist = space.distribution(ids_dev, t_min, t_max)
    assert dist.dtype == torch.float32 and dist.shape == (n, C) and dist.device.type == "cuda"
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    wide = torch.full((n, C + 5), -7.0, device=DEV)
    assert space.distribution(ids_dev, t_min, t_max, out=wide[:, :C]).data_ptr() == wide.data_ptr()
    assert torch.equal(wide[:, :C], dist) and (wide[:, C:] == -7.0).all()
    index, count = space.index(ids_dev, t_min, t_max), space.counts(ids_dev, t_min, t_max)
    assert index.dtype == torch.int64 and np.array_equal(index.cpu().numpy(), want[1])
    assert count.dtype == torch.int64 and np.array_equal(count.cpu().numpy(), want[2])
    return want


@pytest.fixture(scope="module")
def oag_host():
    return TS.oag_graph()


LABEL_TRIPLES = {"PF": ("paper", "field", "PF"), "rev_PF": ("field", "paper", "rev_PF"), "PV": ("paper", "venue", "PV"),
                 "rev_PV": ("venue", "paper", "rev_PV")}


@pytest.mark.parametrize("name, n_cols", [("PF", 1), ("PF", 45), ("PV", 40), ("rev_PF", 1), ("rev_PF", 63), ("rev_PF", 64), ("rev_PF", 65),
                                          ("rev_PF", 1000), ("rev_PV", 64), ("rev_PV", 1000)])
def test_label_kernel_equals_the_numpy_siblings(oag_dev, oag_host, name, n_cols):
    """rows of degree 0 and about 4 (PF, PV: papers), about 530 on both sides of 512 (rev_PF: fields) and about 600 (rev_PV: venues);
    n = 1, 64, 257 rows with repeats and ids outside the type; ids from the host and from the device"""
    triple = LABEL_TRIPLES[name]
    rng = np.random.default_rng(100 + n_cols)
    n_tgt, n_src = TS.OAG_N[triple[0]], TS.OAG_N[triple[1]]
    space = LabelSpace(oag_dev, triple, rng.choice(n_src, n_cols, replace=False))
    assert space.col_of_dev.device.type == "cuda" and (n_cols == n_src or (space.col_of == -1).any())
    deg = np.diff(oag_host.csr[oag_host.triples.index(triple)][0])
    seen = 0
    for n in (1, 64, 257):
        ids = rng.integers(0, n_tgt, size=n)
        if n > 1:
            ids[[0, n // 2, n - 1]] = [n_tgt, int(np.argmin(deg)), -1]
        for window, (t_min, t_max) in TB.WINDOWS.items():
            dev_ids = torch.from_numpy(ids).to(DEV) if window in ("none", "part") else None
            want = _assert_labels(space, oag_host, ids, t_min, t_max, dev_ids)
            seen += int(want[2].sum())
            if n > 1:
                assert want[2][0] == want[2][-1] == 0 and want[1][0] == want[1][-1] == -1
    assert seen > 0
    if name in ("PF", "PV"):
        assert deg.min() == 0 and deg.max() < 64
    else:
        assert deg.max() > 512 and (name == "rev_PV" or deg.min() < 512)


def test_label_kernel_with_a_source_listed_twice_in_a_row():
    host, dev = TB.repeated_source_graph(), TB.repeated_source_graph(device=DEV)
    space = LabelSpace(dev, ("a", "b", "ab"), [5, 3, 1, 4, 2])
    for t_min, t_max in [(None, None), (6, 10), (7, 7), (-5, 5), (None, 6), (8, None)]:
        _assert_labels(space, host, np.arange(4), t_min, t_max)
    assert space.index(torch.arange(4, device=DEV), 6, 10).tolist() == [2, -1, 3, 4]
    assert space.distribution([0], 6, 10).tolist() == [[0, 0.5, 0.5, 0, 0]]
    assert space.distribution(np.zeros(0, np.int64)).shape == (0, 5) and space.index([]).shape == (0,)


def test_label_kernel_with_more_classes_than_one_pass_of_its_bitmap():
    """131072 columns fit the bitmap a workgroup keeps in LDS; 140000 classes take a second pass.  Rows with classes on both sides of
    the line, in the last column of the first pass and the first of the second, and with none"""
    n_b, line = 140000, 131072
    rng = np.random.default_rng(31)
    rows = [[line - 1, line, 5, line - 1], list(rng.choice(n_b, 700, replace=False)), [], [n_b - 1], [0, 1, 2], list(range(line - 40, line + 40))]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    src = np.array([s for r in rows for s in r])
    tm = rng.integers(0, 10, size=src.size)
    feats = {"a": np.zeros((len(rows), 1), np.float32), "b": np.zeros((n_b, 1), np.float32)}
    build = lambda device: DeviceHeteroGraph.from_csr(["a", "b"], [("a", "b", "ab")], {"a": len(rows), "b": n_b}, [(indptr, src, tm)], feats,
                                                      device=device)
    host, dev = build(None), build(DEV)
    space = LabelSpace(dev, ("a", "b", "ab"), np.arange(n_b))          # column = source id
    for t_min, t_max in [(None, None), (3, 6)]:
        want = _assert_labels(space, host, np.arange(len(rows)), t_min, t_max)
    assert want[2].max() > 100
    assert np_label_counts(host, space.triple, space.col_of, np.arange(len(rows))).tolist() == [3, 700, 0, 1, 3, 80]


# ---------------------------------------------------------------------------------------------------------------- failures
def _fail_on_features(dg, call, mask):
    i = dg.types.index("author")
    keep, dg.features[i] = dg.features[i], None
    try:
        with pytest.raises(ValueError, match="no feature matrix"):
            _call(dg, call, mask)
    finally:
        dg.features[i] = keep


def _fail_on_overflow(dg, call, mask):
    st = _device_state(dg, [len(call[0].get(t, [])) for t in dg.types], call[2], call[3])
    i = dg.types.index("author")
    keep, st.types_c[i].cap_cand = st.types_c[i].cap_cand, 5
    try:
        with pytest.raises(RuntimeError, match="overflowed"):
            _call(dg, call, mask)
    finally:
        st.types_c[i].cap_cand = keep


@pytest.mark.parametrize("fail", [_fail_on_features, _fail_on_overflow], ids=["ValueError", "RuntimeError"])
def test_a_failed_masked_call_does_not_poison_the_next_call(oag_dev, fail):
    """a masked call that raises half way, then masked and unmasked calls of another and of the same shape: each equals the host
    sibling"""
    ia, ib = (TS.OAG_CALLS.index(c) for c in TG._SHAPES[:2])
    a, b = TS.OAG_CALLS[ia], TS.OAG_CALLS[ib]
    fail(oag_dev, a, TB.oag_mask(oag_dev, a))
    TG._assert_equals_host(_call(oag_dev, b, TB.oag_mask(oag_dev, b)), _masked_host(oag_dev, ib), oag_dev)
    fail(oag_dev, a, TB.oag_mask(oag_dev, a))
    TG._assert_equals_host(_call(oag_dev, a, TB.oag_mask(oag_dev, a)), _masked_host(oag_dev, ia), oag_dev)
    TG._assert_equals_host(_call(oag_dev, a, None), TG._certified_host(oag_dev, a), oag_dev)
