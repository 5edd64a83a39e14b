"""DeviceHeteroGraph.neighbourhood on the device (csrc/hgt_neighbourhood.hip): every array against the numpy definition, the resident
marks after every call, determinism, the forward on a neighbourhood against the rows of the whole-graph forward, a training step
against float64 on the untrimmed definition graph, and the example."""
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

import neighbourhood_cases as NC
import task_step_cases as TC
import whole_graph_cases as W
from oracle import hgt_oracle as O
from oracle import task_steps as TS
from pyhgt_amd import GNN, Classifier, NeighbourhoodGraph, _lib, label_edge_flags, np_neighbourhood, np_whole_graph
from pyhgt_amd.neighbourhood import NB_CHUNK, NB_WAVE_ROWS
from test_backward_gpu import _grads_close
from test_hgt_gpu import DEV, PREC_TOL
from test_trim_gpu import _make_gnn
from test_whole_graph_gpu import _gnn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _marks_idle(dg):
    assert dg._nb_mark is not None and not dg._nb_dirty
    for t, m in zip(dg.types, dg._nb_mark):
        assert bool((m == -1).all()), "marks of %r are not all -1 after the call" % t


def _host(seeds):
    return {t: (ids.cpu().numpy() if isinstance(ids, torch.Tensor) else ids) for t, ids in seeds.items()}


def _check(dg, seeds, L, what="", **kw):
    """the device result against the definition on the same graph's host CSRs, array for array; the marks are idle afterwards"""
    nb = dg.neighbourhood(seeds, L, **kw)
    torch.cuda.synchronize()
    want = np_neighbourhood(dg, _host(seeds), L, **kw)
    assert isinstance(nb, NeighbourhoodGraph) and nb.gathered and nb.node_feature.is_cuda
    NC.assert_same(NC.graph_arrays(nb), want, what)
    assert nb.host_reads <= L + 1 and nb.n_nodes == want.n_rows[0]
    _marks_idle(dg)
    return nb, want


def test_constants_are_the_library_s():
    c, w, h = (_lib.C.c_int32() for _ in range(3))
    _lib.check(_lib.load().hgt_nb_constants(_lib.C.byref(c), _lib.C.byref(w), _lib.C.byref(h)), "hgt_nb_constants")
    assert (c.value, w.value, h.value) == (_lib.HGT_NB_CHUNK, _lib.HGT_NB_WAVE_ROWS, _lib.HGT_NB_HEAD_WORDS) == (NB_CHUNK, NB_WAVE_ROWS, 40)


# ------------------------------------------------------------------ 1. arrays
def test_hand_graph():
    dg = W.hand_graph(DEV)
    n = 0
    for wt, mt, kind, loops, L, name in itertools.product([False, True], [None, W.HAND_MAX_TIME], [None, "both"], [True, False], [1, 3],
                                                          sorted(NC.HAND_SEEDS)):
        _check(dg, NC.HAND_SEEDS[name], L, (wt, mt, kind, loops, L, name), **NC.hand_kwargs(wt, mt, kind, loops))
        n += 1
    assert n == 128
    _check(dg, NC.HAND_SEEDS["a1_a1_b2"], 2, "targets", **NC.hand_kwargs(True, W.HAND_MAX_TIME, "targets", True))
    _check(dg, NC.HAND_SEEDS["d0"], 2, "sources", **NC.hand_kwargs(True, None, "sources", True))


@pytest.mark.parametrize("kind", ["long_row", "sparse_rows", "multiple_plus_one"])
def test_tile_graphs(kind):
    dg, nested, node_time = W.tile_graph(kind, 512, DEV)
    hub = {"long_row": 3, "sparse_rows": 700, "multiple_plus_one": int(np.argmax(np.diff(dg.csr[0][0])))}[kind]
    for kw in ({}, dict(node_time=node_time, max_time=2001), dict(max_time=2001, self_loops=False)):
        nb, want = _check(dg, {"u": [hub]}, 2, (kind, sorted(kw)), **kw)
    if kind == "long_row":
        nb, _ = _check(dg, {"u": [hub]}, 2)
        assert nb.n_rows == (1061, 1028, 1) and nb.n_edges[1:] == (2115, 1028)


@pytest.fixture(scope="module")
def mag():
    dg, node_time = NC.schema_graph(DEV)
    return dg, node_time


@pytest.mark.parametrize("S,L", [(1, 1), (1, 4), (8, 2), (8, 4), (64, 1), (64, 2), (64, 4)])
def test_mag_schema_graph(mag, S, L):
    dg, node_time = mag
    nb, want = _check(dg, NC.paper_seeds(S), L, (S, L), node_time=node_time)
    if L <= 2:
        assert nb.n_rows[0] < 7680
    if S == 8:
        assert nb.n_rows[0] == {2: 385, 4: 5363}[L]
        flags = label_edge_flags(dg, ["PF_in", "rev_PF_in"], "paper", torch.arange(0, 3000, 7, device=DEV))
        flags_host = {k: tuple(None if f is None else f.cpu().numpy() for f in v) for k, v in flags.items()}
        nb = dg.neighbourhood(NC.paper_seeds(S), L, node_time=node_time, max_time=2012, leave_out=flags)
        NC.assert_same(NC.graph_arrays(nb), np_neighbourhood(dg, NC.paper_seeds(S), L, node_time=node_time, max_time=2012, leave_out=flags_host))
        _marks_idle(dg)


@pytest.mark.parametrize("name", sorted(NC.walk_cases()))
def test_walk_cases(name):
    dg, seeds, L, kw, check = NC.walk_cases(DEV)[name]
    nb, want = _check(dg, seeds, L, name, **kw)
    assert check(NC.graph_arrays(nb)), (name, nb.n_rows, nb.n_edges)


def _fan_graph(n_sources, device, seed=0):
    """u3 has n_sources entries (all of v, in a shuffled stored order, every fifth without a time), u5 a few; every seventh v has a
    source in u: level 1 of {u3} is all of v -- one type -- and level 2 some of u"""
    rng = np.random.default_rng(seed)
    n = {"u": 8, "v": n_sources}
    stamp = lambda: None if rng.random() < 0.2 else int(rng.integers(1995, 2008))
    nested = {("u", "v", "r"): {3: [(int(s), stamp()) for s in rng.permutation(n_sources)],
                                5: [(int(s), stamp()) for s in rng.integers(n_sources, size=3)]},
              ("v", "u", "q"): {i: [(int(rng.integers(8)), stamp())] for i in range(0, n_sources, 7)}}
    node_time = {t: rng.integers(1998, 2006, size=n[t]) for t in n}
    return W.make_graph(["u", "v"], n, list(nested), nested, device), node_time


@pytest.mark.parametrize("n_sources", [NB_WAVE_ROWS, NB_WAVE_ROWS + 1, NB_CHUNK, NB_CHUNK + 1, 3 * NB_CHUNK + 5],
                         ids=["one_wave_of_rows", "one_wave_plus_one", "one_chunk", "one_chunk_plus_one", "three_chunks_and_five"])
def test_sizes_chosen_against_the_kernels(n_sources):
    """a level of exactly one wavefront of rows and one more; a row of exactly one chunk of entries, one more, three chunks and a
    few; level 1 holds one type only; seeds as host lists and as device tensors"""
    dg, node_time = _fan_graph(n_sources, DEV)
    nb, want = _check(dg, {"u": [3]}, 2, "unfiltered")
    assert want.n_rows[1] - want.n_rows[2] == n_sources and set(want.node_type[1:1 + n_sources]) == {1}
    _check(dg, {"u": torch.tensor([3, 5, 3], device=DEV)}, 2, "filtered", node_time=node_time, max_time=2001)
    _check(dg, {"v": torch.arange(n_sources - 1, -1, -1, dtype=torch.int32, device=DEV), "u": [5]}, 1, "a level of seeds", node_time=node_time)
    _check(dg, {"u": np.array([3]), "v": torch.tensor([0, 7])}, 3, "no loops", self_loops=False, max_time=2001)


# ------------------------------------------------------------------ 2. state
def test_state_is_walked_back_after_calls_and_errors(mag):
    dg, node_time = mag
    for S in (3, 17, 40):                                     # three calls in a row, different seeds
        _check(dg, NC.paper_seeds(S), 2, S, node_time=node_time)
    seeds = NC.paper_seeds(8)
    want = np_neighbourhood(dg, seeds, 3, node_time=node_time)
    through_level_2 = want.n_rows[1]
    with pytest.raises(OverflowError, match="level 2") as e:
        dg.neighbourhood(seeds, 3, node_time=node_time, max_rows=through_level_2 - 1)
    assert str(through_level_2) in str(e.value)
    _marks_idle(dg)
    _check(dg, seeds, 3, "after OverflowError", node_time=node_time)
    with pytest.raises(OverflowError, match="edges"):
        dg.neighbourhood(seeds, 3, node_time=node_time, max_time=2015, max_edges=10)
    _marks_idle(dg)
    with pytest.raises(IndexError):                           # a bad seed among good ones, on the device: found by the build
        dg.neighbourhood({"paper": torch.tensor([5, 3000, 7], device=DEV)}, 2, node_time=node_time)
    _marks_idle(dg)
    _check(dg, seeds, 2, "after IndexError", node_time=node_time)
    with pytest.raises(IndexError):
        dg.neighbourhood({"paper": [5, -1]}, 2)
    with pytest.raises(KeyError):
        dg.neighbourhood({"nope": [5]}, 2)
    with pytest.raises(KeyError):
        dg.neighbourhood({"paper": [5]}, 2, leave_out={("paper", "paper", "nope"): (None, None)})
    for L in (0, _lib.HGT_TRIM_MAX_LAYERS + 1):
        with pytest.raises(ValueError):
            dg.neighbourhood({"paper": [5]}, L)
    with pytest.raises(ValueError):
        dg.neighbourhood({"paper": [5]}, 2, node_time={"paper": node_time["paper"]})
    far = dict(node_time, author=node_time["author"] + 500)   # every paper <- author edge has a difference below 0
    with pytest.raises(IndexError):
        dg.neighbourhood(seeds, 2, node_time=far)
    _marks_idle(dg)
    _check(dg, seeds, 2, "after a bad time", node_time=node_time)
    dg._nb_dirty = True                                       # an interrupted call: the next one clears in full
    dg._nb_mark[0][:10] = 7
    _check(dg, seeds, 2, "after an interrupted call", node_time=node_time)


def test_tables_are_kept_by_object_and_later_calls_touch_nothing_of_their_size(mag, monkeypatch):
    """node_time / leave_out tables are validated, converted and uploaded once per OBJECT; a later call with the same objects runs
    none of the per-node checks, makes no further host read and uses the same device tensors; a table changed in place is stale
    until the graph is told to forget it"""
    import pyhgt_amd.neighbourhood as NBM
    dg, _ = mag
    rng = np.random.default_rng(11)
    node_time = {t: rng.integers(2000, 2020, size=n) for t, n in zip(dg.types, dg.n_nodes)}        # host int64: the common form
    flags_host = {("paper", "field_of_study", "PF_in"): (np.arange(3000) % 7 == 0, None)}
    seeds, L = NC.paper_seeds(8), 2
    dg.forget_neighbourhood_tables()
    first = dg.neighbourhood(seeds, L, node_time=node_time, leave_out=flags_host)
    kept = {k: v[1].data_ptr() for k, v in dg._nb_tables.items()}
    assert sorted(k[1] for k in kept) == ["flags"] + ["time"] * 4 and first.host_reads == L + 1
    assert all(v[1].dtype == (torch.int32 if k[1] == "time" else torch.uint8) and v[1].is_cuda for k, v in dg._nb_tables.items())

    def no_validation(*a, **k):
        raise AssertionError("a table the graph has seen was validated again")
    monkeypatch.setattr(NBM, "_node_time_tables", no_validation)
    again = dg.neighbourhood(seeds, L, node_time=node_time, leave_out=flags_host)
    other = dg.neighbourhood(NC.paper_seeds(17), 3, node_time=dict(node_time), leave_out=dict(flags_host))   # new dicts, same arrays
    monkeypatch.undo()
    assert {k: v[1].data_ptr() for k, v in dg._nb_tables.items()} == kept and again.host_reads == L + 1 and other.host_reads == 4
    want = np_neighbourhood(dg, seeds, L, node_time=node_time, leave_out=flags_host)
    NC.assert_same(NC.graph_arrays(first), want)
    NC.assert_same(NC.graph_arrays(again), want)
    # int64 device tables: one host read each (the int32 range) on the call that first sees them, none afterwards
    on_dev = {t: torch.from_numpy(a).to(DEV) for t, a in node_time.items()}
    assert dg.neighbourhood(seeds, L, node_time=on_dev).host_reads == L + 1 + 4
    assert dg.neighbourhood(seeds, L, node_time=on_dev).host_reads == L + 1
    # int32 device tables are taken as they are
    as32 = {t: a.to(torch.int32) for t, a in on_dev.items()}
    nb = dg.neighbourhood(seeds, L, node_time=as32)
    assert nb.host_reads == L + 1 and all(dg._nb_tables[(id(a), "time")][1].data_ptr() == a.data_ptr() for a in as32.values())
    NC.assert_same(NC.graph_arrays(nb), np_neighbourhood(dg, seeds, L, node_time=node_time))
    # a table changed in place keeps its identity: stale until forgotten
    node_time["author"] += 500                                # every paper <- author difference is now below 0
    stale = dg.neighbourhood(seeds, L, node_time=node_time)
    assert stale.n_rows == nb.n_rows and torch.equal(stale.edge_time, nb.edge_time)      # the times of before the change
    dg.forget_neighbourhood_tables()
    assert not dg._nb_tables
    with pytest.raises(IndexError):
        dg.neighbourhood(seeds, L, node_time=node_time)
    _marks_idle(dg)
    with pytest.raises(ValueError):                           # the structural checks run on every call, seen tables or not
        dg.neighbourhood(seeds, L, node_time={"paper": as32["paper"]})
    with pytest.raises(KeyError):
        dg.neighbourhood(seeds, L, node_time=dict(as32, nope=as32["paper"]))
    dg.forget_neighbourhood_tables()


# ------------------------------------------------------------------ 3. determinism
def test_the_same_call_twice_gives_equal_tensors(mag):
    dg, node_time = mag
    seeds = {"paper": torch.from_numpy(NC.paper_seeds(64)["paper"]).to(DEV), "author": [4, 4, 9]}
    a = dg.neighbourhood(seeds, 3, node_time=node_time, max_time=2015)
    b = dg.neighbourhood(seeds, 3, node_time=node_time, max_time=2015)
    assert a.n_rows == b.n_rows and a.n_edges == b.n_edges and a.n_rows[0] > 1000
    for name in NC.FIELDS + ("row_id",):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.seed_rows("paper") == slice(0, 64) and a.seed_rows("author") == slice(64, 67)


# ------------------------------------------------------------------ 4. the forward on a neighbourhood against the whole forward
def _ids(L):
    ids = torch.from_numpy(np.random.default_rng(L).integers(0, 3000, size=300))
    ids[7], ids[100] = ids[3], ids[3]
    return ids


def _forward_case(mag, L, precision, use_rte=True, dense=False, filtered=False):
    dg, node_time = mag
    kw = dict(node_time=node_time if use_rte else None)
    if filtered:
        kw.update(max_time=2012, leave_out=label_edge_flags(dg, ["PF_in", "rev_PF_in"], "paper", torch.arange(0, 3000, 7, device=DEV)))
    view = dg.whole_graph(**kw)
    if dense:
        gnn, _ = _make_gnn(33, 64, 2, L, 4, 9, True, True, use_rte, precision, "dense_hgt", seed=L)
    else:
        sd = O.make_gnn_state_dict(33, 64, 4, 9, 2, L, True, True, use_rte, seed=L)
        gnn = _gnn(sd, 33, 64, 4, 9, 2, L, (True, True), use_rte, precision)
    ids = _ids(L)
    nb = dg.neighbourhood({"paper": ids}, L, **kw)
    with torch.no_grad():
        whole = gnn(*view[:5])
        some = gnn(*nb.inputs, trim=nb)
    torch.cuda.synchronize()
    err = (some - whole[view.type_rows("paper")][ids.to(DEV)]).abs().max().item()
    print("\nL = %d %s%s%s%s: rows %s of %d; max|neighbourhood - whole| %.2e (bound %.0e)"
          % (L, precision, "" if use_rte else " no_rte", " dense" if dense else "", " filtered" if filtered else "", nb.n_rows,
             view[1].numel(), err, PREC_TOL[precision]))
    assert some.shape == (300, 64) and (nb.edge_time is None) == (not use_rte)
    assert err < PREC_TOL[precision], err
    _marks_idle(dg)
    return nb


@pytest.mark.parametrize("L", [1, 2, 4])
def test_forward_on_a_neighbourhood_equals_the_whole_forward(mag, L):
    nb = _forward_case(mag, L, "f16x3")
    if L <= 2:
        assert nb.n_rows[0] < 7680


@pytest.mark.parametrize("case", ["fp32", "bf16x3", "no_rte", "dense", "filtered"])
def test_forward_variants(mag, case):
    kw = dict(fp32=dict(precision="fp32"), bf16x3=dict(precision="bf16x3"), no_rte=dict(precision="f16x3", use_rte=False),
              dense=dict(precision="f16x3", dense=True), filtered=dict(precision="f16x3", filtered=True))[case]
    _forward_case(mag, 2, **kw)


# ------------------------------------------------------------------ 5. a training step against float64 on the untrimmed definition graph
N_OUT, T, R = 7, 4, 9


@pytest.fixture(scope="module")
def world():
    """(released with the module: nothing of it stays on the device for the tests that come after)  A small MAG-schema graph (1 536 nodes), 40 paper seeds with a repeat, labels, and the float64 step on the host on the
    definition's WHOLE graph"""
    L, in_dim, d, H = 2, 33, 64, 2
    dg, node_time = NC.schema_graph(DEV, n_paper=600)
    a = np_whole_graph(dg, node_time=node_time)
    rng = np.random.default_rng(2)
    ids = torch.from_numpy(rng.choice(600, size=40, replace=False))
    ids[7] = ids[2]
    y = torch.from_numpy(rng.integers(0, N_OUT, size=40))
    sd = O.make_gnn_state_dict(in_dim, d, T, R, H, L, True, True, True, seed=L)
    torch.manual_seed(L)
    head_sd = Classifier(d, N_OUT).state_dict()
    P = {k: v.detach().double().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    P.update({"head." + k: v.detach().double().requires_grad_(True) for k, v in head_sd.items()})
    tt = torch.from_numpy
    x64 = tt(a.node_feature).double().requires_grad_(True)
    rep = TS.gnn_rep(P, T, R, H, L, x64, tt(a.node_type), tt(a.edge_time), tt(a.edge_index), tt(a.edge_type))
    loss = torch.nn.functional.nll_loss(TS.classifier(P, rep[ids + a.node_dict["paper"][0]]), y)
    names = [k for k, v in P.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [P[k] for k in names] + [x64], allow_unused=True)
    ref = {k: (torch.zeros_like(P[k]) if g is None else g) for k, g in zip(names, grads)}
    return dict(dg=dg, node_time=node_time, ids=ids, y=y, sd=sd, head_sd=head_sd, ref=ref, ref_x=grads[-1], loss=loss.item(),
                dims=(in_dim, d, H), N=a.node_type.size)


def _train_step(w, L, precision, nb=None, **modes):
    in_dim, d, H = w["dims"]
    gnn = GNN(in_dim, d, T, R, H, L, dropout=0, prev_norm=True, last_norm=True, use_RTE=True, **modes)
    gnn.load_state_dict(w["sd"])
    head = Classifier(d, N_OUT, deterministic=modes.get("deterministic", False))
    head.load_state_dict(w["head_sd"])
    gnn, head = gnn.to(DEV).train(), head.to(DEV).train()
    for gc in gnn.gcs:
        gc.base_conv.precision = precision
    if nb is None:
        nb = w["dg"].neighbourhood({"paper": w["ids"]}, L, node_time=w["node_time"])
    x = nb.node_feature.detach().clone().requires_grad_(True)
    rep = gnn(x, *nb.inputs[1:], trim=nb)
    loss = torch.nn.functional.nll_loss(head(rep), w["y"].to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in list(gnn.named_parameters()) + [("head." + k, v) for k, v in head.named_parameters()]}
    return loss.item(), grads, x.grad, nb


@pytest.mark.parametrize("precision", ["bf16x3", "f16x3"])
def test_training_step_on_a_neighbourhood_against_float64(world, precision):
    L, w = 2, world
    loss, grads, x_grad, nb = _train_step(w, L, precision)
    print("\nloss %.6f, float64 %.6f" % (loss, w["loss"]))
    assert nb.n_rows[0] < w["N"] and set(grads) == set(w["ref"])
    zero = worst = 0
    for name, ref in w["ref"].items():
        g = grads[name]
        if name.endswith("emb.emb.weight") and g is None:       # the fixed sinusoid table (as in tests/task_step_cases.py)
            continue
        if not ref.any():
            assert g is None or not g.detach().cpu().any(), "%s: the float64 gradient is exactly zero, this one is not" % name
            zero += 1
        else:
            assert g is not None, name
            worst = max(worst, _grads_close(name, g, ref, rtol=TC.GRAD_RTOL))
    order = nb.order.cpu()
    outside = torch.ones(w["N"], dtype=torch.bool)
    outside[order] = False
    assert outside.any() and not w["ref_x"][outside].any(), "float64 has a feature gradient outside the neighbourhood"
    err_x = _grads_close("nb.node_feature", x_grad, w["ref_x"][order], rtol=TC.GRAD_RTOL)
    print("\nL=%d %s: rows %s; %d tensors exactly zero, worst %.2e of the largest entry, node_feature %.2e (bound %.0e)"
          % (L, precision, nb.n_rows, zero, worst, err_x, TC.GRAD_RTOL))


def test_deterministic_steps_on_one_neighbourhood_are_bit_identical(world):
    w = world
    _, g1, x1, nb = _train_step(w, 2, "bf16x3", deterministic=True)
    _, g2, x2, _ = _train_step(w, 2, "bf16x3", nb=nb, deterministic=True)
    assert torch.equal(x1, x2)
    for k in g1:
        assert (g1[k] is None and g2[k] is None) or torch.equal(g1[k], g2[k]), k
    _, g3, x3, _ = _train_step(w, 2, "bf16x3", nb=nb, deterministic=True, recompute=True)
    assert torch.equal(x1, x3)
    for k in g1:
        assert (g1[k] is None and g3[k] is None) or torch.equal(g1[k], g3[k]), k


# ------------------------------------------------------------------ 6. the example
def test_example_serves_the_whole_forward_s_predictions():
    spec = importlib.util.spec_from_file_location("serve_exact_ogbn_mag_device", os.path.join(ROOT, "examples", "serve_exact_ogbn_mag_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    res = ex.run(n_paper=2000, n_classes=19, batch=48, n_hid=64, n_heads=2, n_layers=2, seed=1, device=DEV, verbose=False)
    torch.cuda.synchronize()
    assert len(res["served"]) == 48 and res["served"] == res["whole"]
    assert res["rows"][0] < res["graph_nodes"] and res["host_reads"] <= 3
    assert res["max_gap"] < PREC_TOL[res["precision"]]
