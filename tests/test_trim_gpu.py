"""GPU tests of the seed-trimmed forward (run with -m gpu on an MI355X): the device build of the trim against the numpy definition
bit for bit, every trimmed layer against float64 on the UNTRIMMED graph, a training step against torch autograd in float64, and the
degenerate and error cases."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import task_step_cases as TC
from oracle import hgt_oracle as O
from oracle import task_steps as TS
from pyhgt_amd import GNN, Classifier, GraphPlan, _lib, np_trim_graph, np_trim_to_seeds, trim_to_seeds
from pyhgt_amd.sampled import stack_device_graphs, synthetic_sampled_batch, to_device_graph
from pyhgt_amd.synth import induced_in_neighbourhood, synthetic_typed_graph
from test_backward_gpu import _grads_close
from test_gnn_scale_gpu import _gemm_tol
from test_hgt_gpu import DEV, PREC_TOL, _fp64_rows
from test_trim import hand_built_cases

pytestmark = pytest.mark.gpu
HGT_ERR_INVALID_ARG = -1
T, R = 3, 5


# ------------------------------------------------------------------ 1. the arrays equal the definition, bit for bit
def _assert_equals_definition(t, n, ei, et, tm, nt, seeds, L):
    ref = np_trim_to_seeds(n, ei, seeds, L)
    rnt, rei, ret, rtm = np_trim_graph(ref, nt, ei, et, tm)
    torch.cuda.synchronize()
    assert t.n_rows == ref.n_rows and t.n_edges == ref.n_edges and t.n_layers == L
    for name, want in (("hop", ref.hop), ("order", ref.order), ("new_id", ref.new_id), ("edge_order", ref.edge_order),
                       ("node_type", rnt), ("edge_index", rei), ("edge_type", ret), ("edge_time", rtm),
                       ("out_rows", ref.new_id[np.asarray(seeds.cpu() if torch.is_tensor(seeds) else seeds, np.int64).reshape(-1)])):
        got = getattr(t, name)
        if want is None:
            assert got is None, name
            continue
        got = got.cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    return ref


def _dev(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


@pytest.mark.parametrize("name", sorted(hand_built_cases()))
def test_hand_built_cases_equal_the_definition(name):
    n, ei, seeds, L = hand_built_cases()[name]
    E = ei.shape[1]
    nt, et, tm = np.arange(n) % T, np.arange(E) % R, np.arange(E) % 240
    t = trim_to_seeds((_dev(nt), _dev(tm), _dev(ei), _dev(et)), _dev(seeds), L, T, R)
    _assert_equals_definition(t, n, ei, et, tm, nt, seeds, L)


@pytest.mark.parametrize("strided", [True, False], ids=["strided", "contiguous"])
@pytest.mark.parametrize("N,E,S", [(64, 200, 3), (65, 200, 3), (257, 1000, 5), (1500, 6000, 40)])
def test_random_graphs_equal_the_definition(N, E, S, strided):
    """On both sides of a wavefront and of a 256-thread workgroup, and at 1500 nodes (more than one tile of edges), L = 1..4; the
    (1, 2)-strided edge_index of to_torch and a contiguous one; a second trim of the same inputs is identical."""
    _, nt, ei, et, tm = synthetic_typed_graph(N, E, 8, T, R, seed=3, strided_edge_index=strided, device=DEV)
    assert ei.stride() == ((1, 2) if strided else (E, 1))
    seeds = torch.from_numpy(np.random.default_rng(1).integers(0, N, size=S)).to(DEV)
    for L in (1, 2, 3, 4):
        ref = np_trim_to_seeds(N, ei, seeds, L)
        if N == 1500:
            assert ref.n_rows[0] < N, "the case must drop rows"       # (200 / 679 / 1274 / 1446 of 1500)
        t = trim_to_seeds((nt, tm, ei, et), seeds, L, T, R)
        _assert_equals_definition(t, N, ei.cpu().numpy(), et.cpu().numpy(), tm.cpu().numpy(), nt.cpu().numpy(), seeds, L)
        again = trim_to_seeds((nt, None, ei, et), seeds, L, T, R)
        torch.cuda.synchronize()
        assert again.edge_time is None and again.n_rows == t.n_rows and again.n_edges == t.n_edges
        for name in ("hop", "order", "new_id", "edge_order", "node_type", "edge_index", "edge_type", "out_rows"):
            assert torch.equal(getattr(again, name), getattr(t, name)), name


def test_no_edges_no_seeds_and_no_nodes():
    _, nt, ei, et, tm = synthetic_typed_graph(300, 900, 8, T, R, seed=3, device=DEV)
    none = torch.zeros(2, 0, dtype=torch.int64, device=DEV)
    seeds = _dev([7, 299, 7])
    t = trim_to_seeds((nt, tm[:0], none, et[:0]), seeds, 3, T, R)
    _assert_equals_definition(t, 300, np.zeros((2, 0), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), nt.cpu().numpy(), seeds, 3)
    assert t.n_rows == (2, 2, 2, 2) and t.n_edges == (0, 0, 0, 0)
    t = trim_to_seeds((nt, tm, ei, et), seeds[:0], 2, T, R)
    _assert_equals_definition(t, 300, ei.cpu().numpy(), et.cpu().numpy(), tm.cpu().numpy(), nt.cpu().numpy(), seeds[:0], 2)
    assert t.n_rows == (0, 0, 0) and t.n_edges == (0, 0, 0) and t.out_rows.numel() == 0 and bool((t.hop == -1).all())
    t = trim_to_seeds((nt[:0], tm[:0], none, et[:0]), seeds[:0], 1, T, R)
    torch.cuda.synchronize()
    assert t.n_rows == (0, 0) and t.n_edges == (0, 0) and t.order.numel() == 0


# ------------------------------------------------------------------ 2. every trimmed layer against float64 on the untrimmed graph
def _make_gnn(in_dim, d, H, L, n_types, n_rel, prev_norm, last_norm, use_rte, precision, conv, seed):
    torch.manual_seed(seed)
    gnn = GNN(in_dim, d, n_types, n_rel, H, L, 0.2, conv, prev_norm, last_norm, use_rte).eval()
    layer_sd = []
    for li in range(L):
        sd = O.make_state_dict(d, d, n_types, n_rel, H, prev_norm if li < L - 1 else last_norm, use_rte, seed=10 * seed + li,
                               dense=(conv == "dense_hgt"))
        gnn.gcs[li].base_conv.load_state_dict(sd)
        layer_sd.append(sd)
    gnn = gnn.to(DEV)
    for gc in gnn.gcs:
        gc.base_conv.precision = precision
    return gnn, layer_sd


def _fp64_rows_dense(sd, g, targets, x_sub_of):
    """_fp64_rows for DenseHGTConv: the closed form on the sub-graph of all in-edges of the targets, on the host"""
    ids, nts, eis, ets, tms, pos = induced_in_neighbourhood(g["ids"], g["nt"], g["ei"], g["et"], g["tm"] if g["use_rte"] else None, targets)
    xs = x_sub_of(ids.flatten().to(DEV)).cpu()
    out = O.forward_closed_form(sd, g["T"], g["R"], g["H"], xs, nts, eis, ets, tms, use_norm=g["use_norm"], use_RTE=g["use_rte"],
                                dtype=torch.float64, dense=True)
    return out[pos].to(DEV)


def _check_trimmed_stack(gnn, layer_sd, x, nt, tm, ei, et, seeds, n_types, n_rel, H, precision, norms, use_rte, dense=False, tag=""):
    """The trimmed eval forward, stage by stage from the captured input of the stage mapped back through `order`, against float64 on
    the untrimmed graph at the original ids of the stage's rows; rows the trim dropped are NaN in what the reference reads."""
    N, in_dim, d, L = x.size(0), x.size(1), gnn.n_hid, len(gnn.gcs)
    captured = []
    hooks = [gnn.gcs[0].base_conv.register_forward_pre_hook(lambda m, a: captured.append(a[0].detach().clone()))]
    hooks += [gc.base_conv.register_forward_hook(lambda m, a, o: captured.append(o.detach().clone())) for gc in gnn.gcs]
    trim = trim_to_seeds((nt, tm, ei, et), seeds, L, n_types, n_rel)
    with torch.no_grad():
        out = gnn(x, nt, tm, ei, et, trim=trim)
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        by_seeds = gnn(x, nt, tm, ei, et, seeds=seeds)
    torch.cuda.synchronize()
    assert len(captured) == L + 1 and [c.size(0) for c in captured] == list(trim.n_rows)
    assert out.shape == (seeds.numel(), d) and torch.equal(out, captured[L][trim.out_rows]), "the result is not h_L[out_rows]"
    assert torch.equal(by_seeds, out), "seeds= and trim= differ"
    order = trim.order
    # the adapter on rows [0, n_rows[0])
    f16 = precision == "f16x3"
    W = torch.stack([lin.weight.detach() for lin in gnn.adapt_ws]).double()
    b = torch.stack([lin.bias.detach() for lin in gnn.adapt_ws]).double()
    nt0 = nt[order]
    ref0 = torch.zeros(order.numel(), d, dtype=torch.float64, device=DEV)
    for t in range(n_types):
        m = nt0 == t
        ref0[m] = torch.tanh(x[order[m]].double() @ W[t].T + b[t])
    err0 = (captured[0].double() - ref0).abs().max().item()
    unknown = (nt0 < 0) | (nt0 >= n_types)
    assert bool((captured[0][unknown] == 0).all()), "rows of no known type must be exactly 0"
    assert err0 < _gemm_tol(f16, in_dim), err0
    # every layer
    g = dict(T=n_types, R=n_rel, H=H, d=d, ids=torch.arange(N, device=DEV).unsqueeze(1), nt=nt, ei=ei, et=et, tm=tm, use_rte=use_rte,
             deg=torch.bincount(ei[1], minlength=N))
    errs = []
    for l in range(1, L + 1):
        hin = torch.full((N, d), float("nan"), device=DEV)
        hin[order[:trim.n_rows[l - 1]]] = captured[l - 1]
        targets = torch.sort(order[:trim.n_rows[l]]).values
        g["use_norm"] = norms[0] if l < L else norms[1]
        ref = (_fp64_rows_dense if dense else _fp64_rows)(layer_sd[l - 1], g, targets, x_sub_of=lambda ids: hin[ids])
        assert bool(torch.isfinite(ref).all()), "layer %d reads a row the trim dropped" % l
        errs.append((captured[l][trim.new_id[targets]].double() - ref).abs().max().item())
    print("\n%s: rows %s, edges %s; adapter max|err| %.2e (bound %.1e), layers %s (bound %.0e)"
          % (tag, trim.n_rows, trim.n_edges[1:], err0, _gemm_tol(f16, in_dim), ["%.2e" % e for e in errs], PREC_TOL[precision]))
    assert max(errs) < PREC_TOL[precision]
    return trim


def _seeds(N, n=40):
    s = torch.from_numpy(np.random.default_rng(1).integers(0, N, size=n))
    s[5], s[17] = s[3], s[3]                                     # repeated, unsorted
    return s.to(DEV)


STACK_CASES = [
    # n_hid, H, L, use_RTE, (prev_norm, last_norm), precision, conv, planted
    (64, 2, 2, True, (True, True), "f16x3", "hgt", False),
    (64, 2, 4, False, (False, False), "bf16x3", "hgt", False),
    (256, 8, 2, False, (True, False), "bf16x3", "hgt", False),
    (256, 8, 4, True, (False, True), "f16x3", "hgt", False),
    (64, 2, 2, True, (True, True), "fp32", "hgt", False),
    (64, 2, 4, True, (True, True), "f16x3", "dense_hgt", False),
    (256, 8, 2, True, (True, True), "f16x3", "hgt", True),
]


@pytest.mark.parametrize("d,H,L,use_rte,norms,precision,conv,planted", STACK_CASES,
                         ids=["%d-%dl-%s-%s%s" % (c[0], c[2], c[5], c[6], "-planted" if c[7] else "") for c in STACK_CASES])
def test_trimmed_layers_against_fp64_on_the_untrimmed_graph(d, H, L, use_rte, norms, precision, conv, planted):
    N, E, in_dim = 1500, 6000, 33
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, in_dim, T, R, seed=3, device=DEV)
    if planted:
        et[::17] = R + 2                                        # edges no relation claims
        nt[5::37] = T + 1                                       # nodes of no known type
    seeds = _seeds(N)
    if planted:
        seeds[0] = 5                                            # a seed of no known type
    gnn, layer_sd = _make_gnn(in_dim, d, H, L, T, R, norms[0], norms[1], use_rte, precision, conv, seed=L + d)
    GraphPlan.clear_cache()
    trim = _check_trimmed_stack(gnn, layer_sd, x, nt, tm, ei, et, seeds, T, R, H, precision, norms, use_rte, dense=(conv == "dense_hgt"),
                                tag="%s d=%d L=%d %s" % (conv, d, L, precision))
    assert trim.n_rows[0] < N and trim.n_rows[L] == torch.unique(seeds).numel()
    if planted:
        assert int(((trim.node_type < 0) | (trim.node_type >= T)).sum()) > 0 and int((trim.edge_type >= R).sum()) > 0


def test_keep_att_under_a_trim_has_one_row_per_layer_edge():
    N, E, in_dim, d, H, L = 1500, 6000, 33, 64, 2, 2
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, in_dim, T, R, seed=3, device=DEV)
    gnn, _ = _make_gnn(in_dim, d, H, L, T, R, True, True, True, "f16x3", "hgt", seed=1)
    for gc in gnn.gcs:
        gc.base_conv.keep_att = True
    trim = trim_to_seeds((nt, tm, ei, et), _seeds(N), L, T, R)
    with torch.no_grad():
        gnn(x, nt, tm, ei, et, trim=trim)
    for l, gc in enumerate(gnn.gcs, start=1):
        assert gc.base_conv.att.shape == (trim.n_edges[l], H)


def test_trim_of_a_stack_of_three_pieces_through_rows():
    in_dim, d, H, L = 33, 64, 2, 2
    parts = [to_device_graph(*synthetic_sampled_batch("mag", n_seed=8, width=16, depth=2, feat_dim=in_dim, mean_degree=1.5, seed=40 + i),
                             device=DEV, plan=False) for i in range(3)]
    S = stack_device_graphs(parts)
    x, nt, tm, ei, et = S[0], S[1], S[2], S[3], S[4]
    n_types, n_rel = len(S[5]), len(S[6])
    seeds = torch.cat([S.rows(b, "paper", torch.arange(8)) for b in range(3)])
    gnn, layer_sd = _make_gnn(in_dim, d, H, L, n_types, n_rel, True, True, True, "f16x3", "hgt", seed=9)
    trim = _check_trimmed_stack(gnn, layer_sd, x, nt, tm, ei, et, seeds, n_types, n_rel, H, "f16x3", (True, True), True, tag="stack of 3")
    by_graph = trim_to_seeds(S, seeds, L)
    torch.cuda.synchronize()
    assert by_graph.n_rows == trim.n_rows and torch.equal(by_graph.order, trim.order) and by_graph.num_relations == n_rel
    assert trim.n_rows[L] == 24


# ------------------------------------------------------------------ 3. a training step against float64
N_OUT = 7


@functools.lru_cache(maxsize=None)
def _train_world(L):
    """graph, seeds of types 0 and 1 only (the last layer then never computes a row of type 2), labels, the float64 step on the host"""
    N, E, in_dim, d, H = 1500, 6000, 33, 64, 2
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, in_dim, T, R, seed=3)
    rng = np.random.default_rng(2)
    seeds = torch.from_numpy(rng.choice(np.flatnonzero(nt.numpy() != 2), size=40, replace=False))
    seeds[7] = seeds[2]
    y = torch.from_numpy(rng.integers(0, N_OUT, size=40))
    sd = O.make_gnn_state_dict(in_dim, d, T, R, H, L, True, True, True, seed=L)
    torch.manual_seed(L)
    head_sd = Classifier(d, N_OUT).state_dict()
    P = {k: v.detach().double().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    P.update({"head." + k: v.detach().double().requires_grad_(True) for k, v in head_sd.items()})
    x64 = x.double().requires_grad_(True)
    rep = TS.gnn_rep(P, T, R, H, L, x64, nt, tm, ei, et)
    loss = torch.nn.functional.nll_loss(TS.classifier(P, rep[seeds]), y)
    names = [k for k, v in P.items() if v.requires_grad]
    grads = torch.autograd.grad(loss, [P[k] for k in names] + [x64], allow_unused=True)
    ref = {k: (torch.zeros_like(P[k]) if g is None else g) for k, g in zip(names, grads)}
    return dict(x=x, nt=nt, ei=ei, et=et, tm=tm, seeds=seeds, y=y, sd=sd, head_sd=head_sd, ref=ref, ref_x=grads[-1], loss=loss.item(),
                dims=(in_dim, d, H))


def _train_step(w, L, precision, trim=None, x_grad=False, **modes):
    in_dim, d, H = w["dims"]
    gnn = GNN(in_dim, d, T, R, H, L, dropout=0, prev_norm=True, last_norm=True, use_RTE=True, **modes)
    gnn.load_state_dict(w["sd"])
    head = Classifier(d, N_OUT, deterministic=modes.get("deterministic", False))
    head.load_state_dict(w["head_sd"])
    gnn, head = gnn.to(DEV).train(), head.to(DEV).train()
    for gc in gnn.gcs:
        gc.base_conv.precision = precision
    x, nt, ei, et, tm, seeds = (w[k].to(DEV) for k in ("x", "nt", "ei", "et", "tm", "seeds"))
    x.requires_grad_(x_grad)
    if trim is None:
        trim = trim_to_seeds((nt, tm, ei, et), seeds, L, T, R)
    rep = gnn(x, nt, tm, ei, et, trim=trim)
    loss = torch.nn.functional.nll_loss(head(rep), w["y"].to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in list(gnn.named_parameters()) + [("head." + k, v) for k, v in head.named_parameters()]}
    return loss.item(), grads, x.grad, trim


@pytest.mark.parametrize("precision", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("L", [2, 3])
def test_training_step_on_a_trim_against_float64(L, precision):
    w = _train_world(L)
    loss, grads, x_grad, trim = _train_step(w, L, precision, x_grad=True)
    print("\nloss %.6f, float64 %.6f" % (loss, w["loss"]))
    assert trim.n_rows[0] < 1500 and set(grads) == set(w["ref"])
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
    last = "gcs.%d.base_conv." % (L - 1)
    assert not w["ref"][last + "q_linears.2.weight"].any() and zero >= 3, "the case must hold parameters the trimmed graph never touches"
    dropped = (trim.new_id < 0).cpu()
    assert dropped.any() and not x_grad.cpu()[dropped].any(), "a dropped row of node_feature has a gradient"
    assert not w["ref_x"][dropped].any()
    err_x = _grads_close("node_feature", x_grad, w["ref_x"], rtol=TC.GRAD_RTOL)
    print("\nL=%d %s: rows %s; %d tensors exactly zero, worst %.2e of the largest entry, node_feature %.2e (bound %.0e)"
          % (L, precision, trim.n_rows, zero, worst, err_x, TC.GRAD_RTOL))


def test_deterministic_steps_on_one_trim_are_bit_identical():
    w = _train_world(2)
    _, g1, x1, trim = _train_step(w, 2, "bf16x3", x_grad=True, deterministic=True)
    _, g2, x2, _ = _train_step(w, 2, "bf16x3", trim=trim, x_grad=True, deterministic=True)
    assert torch.equal(x1, x2)
    for k in g1:
        assert (g1[k] is None and g2[k] is None) or torch.equal(g1[k], g2[k]), k


def test_recompute_mode_on_a_trim_equals_the_default_mode_bit_for_bit():
    w = _train_world(2)
    _, g1, x1, trim = _train_step(w, 2, "bf16x3", x_grad=True, deterministic=True)
    _, g2, x2, _ = _train_step(w, 2, "bf16x3", trim=trim, x_grad=True, deterministic=True, recompute=True)
    assert torch.equal(x1, x2)
    for k in g1:
        assert (g1[k] is None and g2[k] is None) or torch.equal(g1[k], g2[k]), k


# ------------------------------------------------------------------ 4. degenerate and error cases
def _small(seed=3):
    in_dim, d, H, L = 33, 64, 2, 2
    x, nt, ei, et, tm = synthetic_typed_graph(300, 1200, in_dim, T, R, seed=seed, strided_edge_index=False, device=DEV)
    gnn, layer_sd = _make_gnn(in_dim, d, H, L, T, R, True, True, True, "f16x3", "hgt", seed=2)
    gnn.layer_sd = layer_sd
    return gnn, x, nt, ei, et, tm


def test_a_seed_without_in_edges_and_a_single_seed():
    """A seed without in-edges: one row, every layer edgeless; one seed with in-edges.  Finite, and each stage within the stack's bounds."""
    gnn, x, nt, ei, et, tm = _small()
    lonely = 11
    ei[1][ei[1] == lonely] = 12
    for seed, tag in ((lonely, "a seed without in-edges"), (12, "one seed")):
        seeds = _dev([seed])
        trim = _check_trimmed_stack(gnn, gnn.layer_sd, x, nt, tm, ei, et, seeds, T, R, 2, "f16x3", (True, True), True, tag=tag)
        with torch.no_grad():
            out = gnn(x, nt, tm, ei, et, trim=trim)
        assert out.shape == (1, 64) and bool(torch.isfinite(out).all())
        if seed == lonely:
            assert trim.n_rows == (1, 1, 1) and trim.n_edges == (0, 0, 0)
        else:
            assert trim.n_rows[2] == 1 and trim.n_edges[2] > 0


def test_empty_seeds_give_an_empty_result_and_launch_no_layer():
    gnn, x, nt, ei, et, tm = _small()
    ran = []
    for gc in gnn.gcs:
        gc.base_conv.register_forward_hook(lambda m, a, o: ran.append(1))
    with torch.no_grad():
        out = gnn(x, nt, tm, ei, et, seeds=torch.zeros(0, dtype=torch.int64, device=DEV))
    assert out.shape == (0, 64) and not ran
    x.requires_grad_(True)
    out = gnn.train()(x, nt, tm, ei, et, seeds=torch.zeros(0, dtype=torch.int64, device=DEV))
    assert out.shape == (0, 64) and not ran


def test_errors():
    gnn, x, nt, ei, et, tm = _small()
    seeds = _dev([1, 2, 3])
    for L in (0, _lib.HGT_TRIM_MAX_LAYERS + 1):
        with pytest.raises(ValueError):
            trim_to_seeds((nt, tm, ei, et), seeds, L, T, R)
    with pytest.raises(IndexError):
        trim_to_seeds((nt, tm, ei, et), _dev([1, 300]), 2, T, R)
    with pytest.raises(IndexError):
        trim_to_seeds((nt, tm, ei, et), _dev([-1]), 2, T, R)
    bad = ei.clone()
    bad[0, 77] = 300
    with pytest.raises(IndexError):
        trim_to_seeds((nt, tm, bad, et), seeds, 2, T, R)
    with pytest.raises(ValueError):
        gnn(x, nt, tm, ei, et, trim=trim_to_seeds((nt, tm, ei, et), seeds, 3, T, R))
    with pytest.raises(ValueError):
        gnn(x, nt, tm, ei, et, seeds=seeds, trim=trim_to_seeds((nt, tm, ei, et), seeds, 2, T, R))
    # the C ABI: limits, negative sizes and null pointers answer HGT_ERR_INVALID_ARG and touch nothing
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    need = C.c_uint64()
    assert lib.hgt_trim_tmp_bytes(300, 1200, 2, C.byref(need)) == 0 and need.value > 0
    for args in ((300, 1200, 0), (300, 1200, _lib.HGT_TRIM_MAX_LAYERS + 1), (-1, 0, 2), (0, -1, 2), (2 ** 31, 0, 2), (0, 2 ** 31, 2)):
        assert lib.hgt_trim_tmp_bytes(*args, C.byref(need)) == HGT_ERR_INVALID_ARG, args
    assert lib.hgt_trim_tmp_bytes(300, 1200, 2, None) == HGT_ERR_INVALID_ARG
    assert lib.hgt_trim_tmp_bytes(300, 1200, 2, C.byref(need)) == 0
    tmp = torch.full((int(need.value),), 0x5A, dtype=torch.uint8, device=DEV)
    hops = lambda ei_p, n, e, s_p, s, L, tmp_p: lib.hgt_trim_hops(ei_p, 1200, 1, n, e, s_p, s, L, tmp_p, tmp.numel(), st)
    for args in ((None, 300, 1200, seeds.data_ptr(), 3, 2, tmp.data_ptr()), (ei.data_ptr(), 300, 1200, None, 3, 2, tmp.data_ptr()),
                 (ei.data_ptr(), 300, 1200, seeds.data_ptr(), 3, 2, None), (ei.data_ptr(), 300, 1200, seeds.data_ptr(), 3, 0, tmp.data_ptr()),
                 (ei.data_ptr(), 300, 1200, seeds.data_ptr(), 3, 9, tmp.data_ptr()), (ei.data_ptr(), -1, 1200, seeds.data_ptr(), 3, 2, tmp.data_ptr()),
                 (ei.data_ptr(), 300, -1, seeds.data_ptr(), 3, 2, tmp.data_ptr()), (ei.data_ptr(), 300, 1200, seeds.data_ptr(), -3, 2, tmp.data_ptr()),
                 (ei.data_ptr(), 2 ** 31, 1200, seeds.data_ptr(), 3, 2, tmp.data_ptr())):
        assert hops(*args) == HGT_ERR_INVALID_ARG, args
    out64 = torch.full((8, 1200), -7, dtype=torch.int64, device=DEV)
    hop = torch.full((300,), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((6,), -7, dtype=torch.int32, device=DEV)
    host = torch.full((6,), -7, dtype=torch.int32).pin_memory()

    def fill(L=2, n=300, counts_p=counts.data_ptr(), host_p=host.data_ptr(), order_p=out64[0].data_ptr(), nt_p=nt.data_ptr()):
        return lib.hgt_trim_fill(ei.data_ptr(), 1200, 1, et.data_ptr(), tm.data_ptr(), nt_p, n, 1200, seeds.data_ptr(), 3, L, tmp.data_ptr(),
                                 tmp.numel(), hop.data_ptr(), order_p, out64[1].data_ptr(), out64[2].data_ptr(), out64[3].data_ptr(),
                                 out64[4].data_ptr(), out64[6].data_ptr(), out64[7].data_ptr(), out64[3, 600:].data_ptr(), counts_p, host_p, st)

    for kw in (dict(L=0), dict(L=9), dict(n=-1), dict(n=2 ** 31), dict(counts_p=None), dict(host_p=None), dict(order_p=None), dict(nt_p=None)):
        assert fill(**kw) == HGT_ERR_INVALID_ARG, kw
    torch.cuda.synchronize()
    assert bool((tmp == 0x5A).all()) and bool((out64 == -7).all()) and bool((hop == -7).all()) and bool((counts == -7).all())
    assert bool((host == -7).all())
