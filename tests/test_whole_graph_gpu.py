"""GPU tests of the whole-graph view (run with -m gpu on an MI355X): the device build against the numpy definition element for
element, the layers on a view against float64 on the definition's tensors, exact inference through seeds=, a filtered view through a
layer, and the example."""
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

from oracle import hgt_oracle as O
from pyhgt_amd import GNN, GraphPlan, _lib, label_edge_flags, np_whole_graph
from pyhgt_amd.sampled import MAG_META, OAG_META
from pyhgt_amd.sampler import DeviceHeteroGraph
from pyhgt_amd.synth import synthetic_hetero_csr
from pyhgt_amd.view import VIEW_TILE
from test_gnn_scale_gpu import _gemm_tol
from test_hgt_gpu import DEV, PREC_TOL

import whole_graph_cases as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAG_TYPES = ["paper", "author", "field_of_study", "institution"]
OAG_TYPES = ["paper", "author", "field", "venue", "affiliation"]


# ------------------------------------------------------------------ 5. the arrays equal the definition, element for element
def _assert_equals_definition(view, a):
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    for name, got, want in [("sorted[%d]" % i, host(g), w) for i, (g, w) in enumerate(zip(view.sorted, a.sorted))] + \
                           [(n, host(view[i]), a[i]) for i, n in enumerate(("node_feature", "node_type", "edge_time", "edge_index", "edge_type"))]:
        if want is None:
            assert got is None, name
            continue
        assert got is not None and got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    assert view[5] == a.node_dict and view[6] == a.edge_dict
    assert view.sorted[0].is_contiguous() and view.sorted[3].numel() == len(a.edge_dict) + 1


def _both(dg_dev, dg_host, **kw):
    view = dg_dev.whole_graph(plan=False, **kw)
    a = np_whole_graph(dg_host, **kw)
    _assert_equals_definition(view, a)
    view.raise_if_bad(wait=True)
    return view, a


@pytest.mark.parametrize("flags", [None, "targets", "sources", "both"])
def test_hand_made_graph_equals_the_definition(flags):
    """the cases of tests/test_whole_graph.py (shared relation name, empty type, empty triples, empty rows, None times) on the device"""
    dev, host = W.hand_graph(DEV), W.hand_graph()
    leave_out = None if flags is None else W.hand_flags(flags)
    for with_time, max_time, self_loops in itertools.product([True, False], [None, W.HAND_MAX_TIME, 1900], [True, False]):
        view, a = _both(dev, host, node_time=W.HAND_TIME if with_time else None, max_time=max_time, leave_out=leave_out, self_loops=self_loops)
        edges, rel_ptr = W.brute_force(host, W.HAND_NESTED, W.HAND_TIME if with_time else None, max_time, leave_out, self_loops)
        assert view[3].size(1) == len(edges) and view.sorted[3].tolist() == rel_ptr


@pytest.mark.parametrize("kind", ["long_row", "multiple", "multiple_plus_one", "sparse_rows"])
def test_tile_shaped_graphs_equal_the_definition(kind):
    """Against the build's tile (VIEW_TILE = %d entries per wavefront, four tiles per workgroup): a row of 2 * tile + 3 neighbours
    followed by rows of one; all entries an exact multiple of the tile, and one more; stretches of rows without an entry longer than
    the walk follows.  Unfiltered, and filters that keep everything, nothing and about half; flags on targets, sources, both."""
    dev, _, node_time = W.tile_graph(kind, VIEW_TILE, DEV)
    host, _, _ = W.tile_graph(kind, VIEW_TILE)
    total = sum(c[1].size for c in host.csr) + sum(host.n_nodes)
    if kind == "multiple":
        assert total == 8 * VIEW_TILE
    if kind == "multiple_plus_one":
        assert total == 8 * VIEW_TILE + 1
    if kind == "long_row":
        assert np.diff(host.csr[0][0]).max() == 2 * VIEW_TILE + 3
    N = sum(host.n_nodes)
    for with_time in (True, False):
        nt = node_time if with_time else None
        _both(dev, host, node_time=nt)
        _both(dev, host, node_time=nt, self_loops=False)
        v, _ = _both(dev, host, node_time=nt, max_time=3000)
        assert v[3].size(1) == total
        v, _ = _both(dev, host, node_time=nt, max_time=2000)
        assert N < v[3].size(1) < total
    v, _ = _both(dev, host, node_time=node_time, max_time=1900)
    assert v[3].size(1) == N                                           # nothing but the self loops
    rng = np.random.default_rng(7)
    fu, fv = rng.random(host.n_nodes[0]) < 0.5, (rng.random(host.n_nodes[1]) < 0.5).astype(np.uint8)
    sides = {"targets": {("u", "v", "r0"): (fu, None), ("v", "u", "r1"): (fv, None)},
             "sources": {("u", "v", "r0"): (None, fv), ("u", "u", "r2"): (None, fu)},
             "both": {("u", "v", "r0"): (fu, fv), ("v", "u", "r1"): (fv, fu), ("u", "u", "r2"): (fu, fu)}}
    for leave_out in sides.values():
        v, _ = _both(dev, host, node_time=node_time, leave_out=leave_out)
        assert N < v[3].size(1) < total
        _both(dev, host, leave_out=leave_out, max_time=2000, self_loops=False)


test_tile_shaped_graphs_equal_the_definition.__doc__ %= VIEW_TILE


def test_every_other_entry_is_kept():
    """stored times that alternate around max_time: every wavefront ballot has every other bit set"""
    host, _, node_time = W.tile_graph("multiple_plus_one", VIEW_TILE)
    csr = [(ip, src, (2000 + 10 * (np.arange(src.size) % 2)).astype(np.int32)) for ip, src, _ in host.csr]
    n_nodes = dict(zip(host.types, host.n_nodes))
    feats = dict(zip(host.types, host.features_host))
    make = lambda device: DeviceHeteroGraph.from_csr(host.types, host.meta, n_nodes, csr, feats, device=device)
    v, _ = _both(make(DEV), make(None), node_time=node_time, max_time=2005)
    assert v[3].size(1) == sum((c[1].size + 1) // 2 for c in csr) + sum(host.n_nodes)


@pytest.mark.parametrize("self_loops", [True, False])
def test_single_node(self_loops):
    """one node without edges; without self loops the view has no edge at all"""
    make = lambda device: DeviceHeteroGraph.from_csr(["u"], [("u", "u", "r")], {"u": 1}, [(np.zeros(2, np.int32), np.zeros(0, np.int32), None)],
                                                     {"u": np.ones((1, 4), np.float32)}, device=device)
    for kw in (dict(), dict(node_time={"u": np.array([2000])}), dict(max_time=1999), dict(node_time={"u": np.array([2000])}, max_time=1999)):
        v, _ = _both(make(DEV), make(None), self_loops=self_loops, **kw)
        assert v[3].shape == (2, 1 if self_loops else 0) and v.sorted[3].tolist() == [0, 0, 1 if self_loops else 0]


def test_device_arguments_and_errors():
    """node_time, flags and ids as device tensors; the errors of the definition; an out-of-range time difference is an IndexError
    -- at once from a filtered view, from `raise_if_bad` of an unfiltered one built without a plan (with a plan: the next test)"""
    dev, host = W.hand_graph(DEV), W.hand_graph()
    nt_dev = {t: torch.from_numpy(v).to(DEV) for t, v in W.HAND_TIME.items()}
    lo = W.hand_flags("both")
    lo_dev = {tri: tuple(None if f is None else torch.from_numpy(np.asarray(f)).to(DEV) for f in pair) for tri, pair in lo.items()}
    _assert_equals_definition(dev.whole_graph(nt_dev, W.HAND_MAX_TIME, lo_dev, plan=False), np_whole_graph(host, W.HAND_TIME, W.HAND_MAX_TIME, lo))
    ids = [3, 5]
    by_dev = label_edge_flags(dev, ["x", "link"], "a", torch.tensor(ids, device=DEV))
    by_host = label_edge_flags(host, ["x", "link"], "a", ids)
    assert all(f is None or f.is_cuda for pair in by_dev.values() for f in pair)
    _assert_equals_definition(dev.whole_graph(leave_out=by_dev, plan=False), np_whole_graph(host, leave_out=by_host))
    assert label_edge_flags(dev, ["x"], "a", ids)[("a", "a", "x")][0].cpu().tolist() == [0, 0, 0, 1, 0, 1]
    with pytest.raises(ValueError):
        dev.whole_graph(node_time={"a": W.HAND_TIME["a"]})
    with pytest.raises(KeyError):
        dev.whole_graph(leave_out={("a", "d", "link"): (None, None)})
    late = dict(W.HAND_TIME, b=W.HAND_TIME["b"] + 121)
    with pytest.raises(IndexError):
        dev.whole_graph(node_time=late, max_time=3000, plan=False)
    view = dev.whole_graph(node_time=late, plan=False)
    with pytest.raises(IndexError):
        view.raise_if_bad(wait=True)
    dev.whole_graph(node_time=W.HAND_TIME, plan=False).raise_if_bad(wait=True)
    with pytest.raises(RuntimeError):
        DeviceHeteroGraph.from_csr(["u"], [("u", "u", "r")], {"u": 1}, [(np.zeros(2, np.int32), np.zeros(0, np.int32), None)],
                                   {"u": np.ones((1, 4), np.float32)}, device="cpu").whole_graph()


def test_bad_time_of_an_unfiltered_view_raises_from_the_plan_and_the_forward():
    """An unfiltered view is built without a host read, so a time difference outside [0, 240) cannot raise from `whole_graph`.  It
    must not pass through the model either: edge_time carries the value as it is, the plan flags it in its header, and
    `plan.raise_if_bad` / a strict layer's forward raise the reference's IndexError.  With use_RTE=False the layer never looks at
    edge_time and runs.  int64 device node times beyond int32 are refused, not wrapped."""
    n = {"u": 700, "v": 300}
    meta = [("u", "v", "r0"), ("v", "u", "r1")]
    csr = synthetic_hetero_csr(["u", "v"], meta, n, mean_degree=3.0, seed=4)
    rng = np.random.default_rng(5)
    feats = {t: rng.standard_normal((n[t], 16)).astype(np.float32) for t in n}
    dev = DeviceHeteroGraph.from_csr(["u", "v"], meta, n, csr, feats, device=DEV)
    host = DeviceHeteroGraph.from_csr(["u", "v"], meta, n, csr, feats)
    good = {"u": rng.integers(2000, 2020, size=700), "v": rng.integers(2000, 2020, size=300)}
    bad = dict(good, v=good["v"].copy())
    target = int(np.flatnonzero(np.diff(host.csr[0][0]) > 0)[0])                  # a u node with a v neighbour
    nb = int(host.csr[0][1][host.csr[0][0][target]])
    bad["v"][nb] = good["u"][target] - 125                                        # 125 + 120 >= 240
    with pytest.raises(IndexError):
        np_whole_graph(host, node_time=bad)
    GraphPlan.clear_cache()
    view = dev.whole_graph(node_time=bad)                                          # plan=True
    torch.cuda.synchronize()
    assert int(view[2].max()) >= 240 and int(view.sorted[2].max()) == int(view[2].max()), "edge_time must carry the value as it is"
    with pytest.raises(IndexError):
        view.plan.raise_if_bad(wait=True)
    with pytest.raises(IndexError):
        view.raise_if_bad(wait=True)
    sd = O.make_gnn_state_dict(16, 32, 2, 3, 2, 2, True, True, True, seed=1)
    gnn = _gnn(sd, 16, 32, 2, 3, 2, 2, (True, True), True, "f16x3")
    GraphPlan.clear_cache()
    fresh = dev.whole_graph(node_time=bad)
    for gc in gnn.gcs:
        gc.base_conv.strict = True
    with pytest.raises(IndexError), torch.no_grad():
        gnn(*fresh[:5])
    GraphPlan.clear_cache()
    lazy = dev.whole_graph(node_time=bad)                                          # not strict: the flag lands, the next forward raises
    for gc in gnn.gcs:
        gc.base_conv.strict = False
    torch.cuda.synchronize()
    with pytest.raises(IndexError), torch.no_grad():
        gnn(*lazy[:5])
    sd0 = O.make_gnn_state_dict(16, 32, 2, 3, 2, 2, True, True, False, seed=1)
    plain = _gnn(sd0, 16, 32, 2, 3, 2, 2, (True, True), False, "f16x3")
    with torch.no_grad():
        assert bool(torch.isfinite(plain(*lazy[:5])).all())                        # (conv.py:91: no RTE, edge_time is not read)
    ok = dev.whole_graph(node_time=good)
    ok.plan.raise_if_bad(wait=True)
    ok.raise_if_bad(wait=True)
    with pytest.raises(ValueError):
        dev.whole_graph(node_time={"u": torch.from_numpy(good["u"]).to(DEV) + 2 ** 33, "v": torch.from_numpy(good["v"]).to(DEV)})


# ------------------------------------------------------------------ 6. layers on the view against float64
def _schema_graph(types, meta, n_paper, frac, in_dim, seed, none_time, mean_degree=3.0):
    n_nodes = {t: max(4, int(n_paper * f)) for t, f in zip(types, frac)}
    csr = synthetic_hetero_csr(types, meta, n_nodes, mean_degree=mean_degree, seed=seed, years=(2000, 2020), none_time=none_time)
    rng = np.random.default_rng(seed + 1)
    feats = {t: rng.standard_normal((n_nodes[t], in_dim)).astype(np.float32) for t in types}
    node_time = {t: rng.integers(2000, 2020, size=n_nodes[t]) for t in types}
    return (DeviceHeteroGraph.from_csr(types, meta, n_nodes, csr, feats, device=DEV), DeviceHeteroGraph.from_csr(types, meta, n_nodes, csr, feats),
            node_time)


@pytest.fixture(scope="module")
def mag():
    return _schema_graph(MAG_TYPES, MAG_META, 3000, [1.0, 1.5, 0.05, 0.01], 33, 3, ("AI_in",))


def _gnn(sd, in_dim, d, T, R, H, L, norms, use_rte, precision):
    gnn = GNN(in_dim, d, T, R, H, L, 0.2, "hgt", norms[0], norms[1], use_rte).eval()
    gnn.load_state_dict(sd)
    gnn = gnn.to(DEV)
    for gc in gnn.gcs:
        gc.base_conv.precision = precision
    return gnn


def _check_stack_on(view, a, sd, in_dim, d, H, L, norms, use_rte, precision, rows, tag):
    """the eval forward on the view, stage by stage, against float64 on the DEFINITION's tensors: the adapter is
    oracle.gnn_forward with no layer, a layer is the closed form gnn_forward applies, from the captured input of the stage; compared
    at `rows`"""
    T, R = len(a.node_dict), len(a.edge_dict)
    gnn = _gnn(sd, in_dim, d, T, R, H, L, norms, use_rte, precision)
    captured = []
    hooks = [gnn.gcs[0].base_conv.register_forward_pre_hook(lambda m, args: captured.append(args[0].detach().clone()))]
    hooks += [gc.base_conv.register_forward_hook(lambda m, args, o: captured.append(o.detach().clone())) for gc in gnn.gcs]
    tm_view = view[2] if use_rte else None
    with torch.no_grad():
        out = gnn(view[0], view[1], tm_view, view[3], view[4])
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert out.shape == (a.node_type.size, d) and len(captured) == L + 1
    tt = torch.from_numpy
    nf, nt, ei, et = tt(a.node_feature), tt(a.node_type), tt(a.edge_index), tt(a.edge_type)
    tm = tt(a.edge_time) if use_rte else None
    ref0 = O.gnn_forward(sd, in_dim, d, T, R, H, 0, norms[0], norms[1], use_rte, nf, nt, tm, ei, et)
    err0 = (captured[0].cpu().double() - ref0).abs().max().item()
    errs = []
    for l in range(L):
        pre = "gcs.%d.base_conv." % l
        lsd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        ref = O.forward_closed_form(lsd, T, R, H, captured[l].cpu().double(), nt, ei, et, tm, use_norm=norms[0] if l < L - 1 else norms[1],
                                    use_RTE=use_rte, dtype=torch.float64)
        errs.append((captured[l + 1].cpu().double()[rows] - ref[rows]).abs().max().item())
    print("\n%s: %d nodes, %d edges; adapter max|err| %.2e (bound %.1e), layers %s (bound %.0e)"
          % (tag, nt.numel(), ei.size(1), err0, _gemm_tol(precision == "f16x3", in_dim), ["%.2e" % e for e in errs], PREC_TOL[precision]))
    assert err0 < _gemm_tol(precision == "f16x3", in_dim), err0
    assert max(errs) < PREC_TOL[precision], errs
    return gnn, out


@pytest.mark.parametrize("use_rte", [True, False], ids=["rte", "no_rte"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "f16x3"])
def test_layers_on_the_view_against_fp64(mag, precision, use_rte):
    dev, host, node_time = mag
    in_dim, d, H, L, norms = 33, 64, 2, 2, (True, True)
    GraphPlan.clear_cache()
    view = dev.whole_graph(node_time=node_time if use_rte else None)
    a = np_whole_graph(host, node_time=node_time if use_rte else None)
    T, R = len(a.node_dict), len(a.edge_dict)
    assert (T, R) == (4, 9) and (view[2] is None) == (not use_rte)
    assert GraphPlan.cached(view[1], view[3], view[4], view[2], T, R) is view.plan, "the registered plan is not the one a layer finds"
    sd = O.make_gnn_state_dict(in_dim, d, T, R, H, L, norms[0], norms[1], use_rte, seed=5)
    rows = torch.from_numpy(np.random.default_rng(2).choice(a.node_type.size, size=600, replace=False))
    _check_stack_on(view, a, sd, in_dim, d, H, L, norms, use_rte, precision, rows, "mag-%s-%s" % (precision, "rte" if use_rte else "no_rte"))
    view.plan.raise_if_bad(wait=True)


def test_plan_of_more_than_4096_tile_relation_pairs():
    """An OAG-schema view of about 32 k nodes: its (destination tile, relation) table has more than 4096 entries, so
    hgt_plan_from_sorted builds the plan with its multi-launch branch; the layers on it against float64 as above"""
    dev, host, node_time = _schema_graph(OAG_TYPES, OAG_META, 12500, [1.0, 1.5, 0.05, 0.005, 0.02], 17, 9, ("in",), mean_degree=0.25)
    tile, item = _lib.C.c_int32(), _lib.C.c_int32()
    _lib.check(_lib.load().hgt_plan_constants(_lib.C.byref(tile), _lib.C.byref(item)), "hgt_plan_constants")
    view, a = dev.whole_graph(node_time=node_time), np_whole_graph(host, node_time=node_time)
    N, R = a.node_type.size, len(a.edge_dict)
    n_pairs = (N + tile.value - 1) // tile.value * (R + 1)
    assert n_pairs + 1 > 4096 and N < 40000, (N, n_pairs)
    in_dim, d, H, L, norms = 17, 32, 2, 2, (True, True)
    sd = O.make_gnn_state_dict(in_dim, d, len(a.node_dict), R, H, L, norms[0], norms[1], True, seed=6)
    rows = torch.from_numpy(np.random.default_rng(2).choice(N, size=600, replace=False))
    _check_stack_on(view, a, sd, in_dim, d, H, L, norms, True, "f16x3", rows, "oag-%d-pairs" % n_pairs)
    view.plan.raise_if_bad(wait=True)
    _assert_equals_definition(view, a)


# ------------------------------------------------------------------ 7. exact inference through seeds=
@pytest.mark.parametrize("L", [1, 2, 4])
def test_exact_inference_of_a_set_of_nodes(mag, L):
    """gnn(*view[:5], seeds=view.rows("paper", ids)) against the rows `ids` of the whole forward: ids with repeats, in no order"""
    dev, _, node_time = mag
    precision = "f16x3"
    view = dev.whole_graph(node_time=node_time)
    sd = O.make_gnn_state_dict(33, 64, 4, 9, 2, L, True, True, True, seed=L)
    gnn = _gnn(sd, 33, 64, 4, 9, 2, L, (True, True), True, precision)
    ids = torch.from_numpy(np.random.default_rng(L).integers(0, 3000, size=300))
    ids[7], ids[100] = ids[3], ids[3]
    with torch.no_grad():
        whole = gnn(*view[:5])
        some = gnn(*view[:5], seeds=view.rows("paper", ids))
    torch.cuda.synchronize()
    assert torch.equal(view.rows("paper", ids).cpu(), ids + view.type_rows("paper").start) and view.rows("author").numel() == 4500
    err = (some - whole[view.type_rows("paper")][ids.to(DEV)]).abs().max().item()
    print("\nL = %d: max|seeds - whole| %.2e (bound %.0e)" % (L, err, PREC_TOL[precision]))
    assert some.shape == (300, 64) and err < PREC_TOL[precision]


# ------------------------------------------------------------------ 8. a filtered view through a layer
def test_filtered_view_through_the_layers(mag):
    """max_time plus leave_out: the layers against float64 on the definition's FILTERED tensors, and a left-out label edge changes
    the output of its target against the unfiltered view"""
    dev, host, node_time = mag
    precision, in_dim, d, H, L, norms = "f16x3", 33, 64, 2, 2, (True, True)
    labelled = np.arange(0, 3000, 7)
    flags = label_edge_flags(dev, ["PF_in", "rev_PF_in"], "paper", torch.from_numpy(labelled).to(DEV))
    flags_host = label_edge_flags(host, ["PF_in", "rev_PF_in"], "paper", labelled)
    view = dev.whole_graph(node_time=node_time, max_time=2012, leave_out=flags)
    a = np_whole_graph(host, node_time=node_time, max_time=2012, leave_out=flags_host)
    full = np_whole_graph(host, node_time=node_time)
    assert 7680 < a.edge_type.size < full.edge_type.size and view.filtered
    _assert_equals_definition(view, a)
    sd = O.make_gnn_state_dict(in_dim, d, 4, 9, H, L, norms[0], norms[1], True, seed=8)
    rows = torch.from_numpy(np.random.default_rng(3).choice(a.node_type.size, size=600, replace=False))
    gnn, out = _check_stack_on(view, a, sd, in_dim, d, H, L, norms, True, precision, rows, "mag-filtered")
    # the filter reaches the layer: a paper that lost a label edge (and nothing else) has another output
    only = dev.whole_graph(node_time=node_time, leave_out=flags)
    plain = dev.whole_graph(node_time=node_time)
    m = host.triples.index(("paper", "field_of_study", "PF_in"))
    deg = np.diff(host.csr[m][0])
    target = int(labelled[np.flatnonzero(deg[labelled] > 0)[0]])
    with torch.no_grad():
        with_edge, without = gnn(*plain[:5])[target], gnn(*only[:5])[target]
    assert only[3].size(1) == plain[3].size(1) - 2 * int(deg[labelled].sum())
    assert (with_edge - without).abs().max().item() > 100 * PREC_TOL[precision]


# ------------------------------------------------------------------ 9. the example
def test_example_exact_evaluation():
    spec = importlib.util.spec_from_file_location("eval_whole_graph_ogbn_mag_device", os.path.join(ROOT, "examples", "eval_whole_graph_ogbn_mag_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res = ex.run(steps=2, n_paper=2000, n_classes=19, batch_size=64, seed=1, device=DEV, verbose=False, n_hid=64, n_heads=2, depth=2, width=32,
                 vr_num=2)
    torch.cuda.synchronize()
    logits, y, split = (res["exact"][k].cpu().numpy() for k in ("logits", "y", "split"))
    pred = logits.argmax(axis=1)
    top2 = np.sort(logits, axis=1)[:, -2:]
    assert (top2[:, 1] > top2[:, 0]).all(), "a tie in the logits: argmax is not defined count for count"
    want = [[int((split == s).sum()), int(((split == s) & (pred == y)).sum())] for s in range(3)]
    assert res["exact"]["counts"] == want and sum(n for n, _ in want) == 2000
    assert res["exact"]["accuracy"] == [c / n for n, c in want]
    assert set(res["voted"]) == {"variance_reduce", "sequential"} and len(res["losses"]) == 2
    c = res["chunk"]
    err = (c["seeds_out"] - c["whole_out"]).abs().max().item()
    assert c["seeds_out"].shape == (64, 64) and err < PREC_TOL[res["precision"]], err
