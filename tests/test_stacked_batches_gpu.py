"""Stacked batches on the GPU: `stack_device_graphs` (hgt_stack_sorted + hgt_gather_rows + hgt_plan_from_sorted) against the host
merge handed over the usual way, the layers on the stacked graph against the fp64 oracle and against the pieces run alone, a
training step against the fp64 backward and the sum of the separate steps, and the two ways it can be misused.  The piece sets
and the numpy restatement of the stacked order live in tests/test_stacked_batches.py."""
import numpy as np
import pytest
import torch

import test_backward_gpu as BG
import test_stacked_batches as SB
from oracle import hgt_oracle as O
from pyhgt_amd import GNN, Classifier, GraphPlan, HGTConv
from pyhgt_amd.sampled import (_DeviceGraph, merge_sampler_outputs, stack_device_graphs, synthetic_sampled_batch,
                               to_device_graph)
from test_hgt_gpu import DEV, PREC_TOL, _fp64_rows, _plan_arrays

pytestmark = pytest.mark.gpu

PLAN_ARRAYS = ("esrc", "edst", "ertei", "eid", "segptr", "tile_items", "rows_all", "off_all", "rows_q", "off_q")


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and torch.equal(a, b))


def _check_layout(pieces):
    """stack_device_graphs(pieces on the device) == to_device_graph(merge_sampler_outputs(pieces)): the five tensors, the
    dictionaries, the sorted int32 form, every array of the plan; the maps are the permutations of the restatement."""
    GraphPlan.clear_cache()
    parts = [to_device_graph(*p, device=DEV, plan=(i % 2 == 0)) for i, p in enumerate(pieces)]
    S = stack_device_graphs(parts)
    M = to_device_graph(*merge_sampler_outputs(pieces), device=DEV)
    torch.cuda.synchronize()
    names = ("node_feature", "node_type", "edge_time", "edge_index", "edge_type")
    for i, name in enumerate(names):
        assert _same(S[i], M[i]), name
    assert S[5] == M[5] and S[6] == M[6]
    assert S[3].shape[0] == 2 and S[3].stride() == M[3].stride()
    for a, b in zip(S.sorted, M.sorted):
        assert _same(a, b)
    a, b = _plan_arrays(S.plan), _plan_arrays(M.plan)
    assert a["bad"] == 0 and b["bad"] == 0
    for k in ("n_items", "n_bins"):
        assert a[k] == b[k], k
    for k in PLAN_ARRAYS:      # (compared array by array: the 256-byte padding between them is never written)
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["items"][:a["n_items"]].tobytes() == b["items"][:b["n_items"]].tobytes()
    want = SB.restate_sorted([SB.sorted_numpy(g) for g in parts])
    node_map, edge_map = S.node_map.cpu().numpy(), S.edge_map.cpu().numpy()
    assert node_map.dtype == np.int32 and edge_map.dtype == np.int32
    assert np.array_equal(np.sort(node_map), np.arange(S[1].numel())) and np.array_equal(np.sort(edge_map), np.arange(S[4].numel()))
    assert np.array_equal(node_map, want["node_map"]) and np.array_equal(edge_map, want["edge_map"])
    # the ways back to the pieces
    T, R = len(S[5]), len(S[6])
    assert S.n_graphs == len(pieces) and GraphPlan.cached(S[1], S[3], S[4], S[2], T, R) is S.plan
    types = pieces[0][3].get_types()
    _, _, new_id = SB.restate_nodes([SB.sorted_numpy(g)[4] for g in parts])
    for b, g in enumerate(parts):
        assert torch.equal(S.unstack(S[0])[b], g[0])
        off = SB.sorted_numpy(g)[4]
        for t, name in enumerate(types):
            assert np.array_equal(S.rows(b, name).cpu().numpy(), new_id[b][off[t]:off[t + 1]])
        n_paper = int(off[1] - off[0])
        pick = torch.arange(0, n_paper, 3)
        assert np.array_equal(S.rows(b, "paper", pick).cpu().numpy(), new_id[b][:n_paper][::3])
    return parts, S


LAYOUT_SETS = {
    "mag": lambda: SB.piece_set("mag"), "oag": lambda: SB.piece_set("oag"), "tiny33": SB.tiny_pieces,
    "one": lambda: SB.piece_set("mag")[1:2], "mag-no-time": lambda: SB.without_time(SB.piece_set("mag")),
    "oag-no-time": lambda: SB.without_time(SB.piece_set("oag")),
}


@pytest.mark.parametrize("which", list(LAYOUT_SETS))
def test_stacked_layout_equals_the_merged_hand_off(which):
    """Pieces with an empty type, a missing relation, only `self` edges; one piece; 33 pieces of the 33-relation schema; with
    and without edge_time."""
    pieces = LAYOUT_SETS[which]()
    parts, S = _check_layout(pieces)
    assert (S[2] is None) == which.endswith("no-time")
    if which == "one":
        for a, b in zip(S[:5], parts[0][:5]):
            assert _same(a, b)
    # a stack can be stacked again: inside a type (and inside a (relation, target type)) the pieces of (A + B) + C follow each
    # other as in A + B + C, so the result is the same graph in the same order
    if which == "mag":
        again = stack_device_graphs([stack_device_graphs(parts[:2]), parts[2]])
        assert again.n_graphs == 2
        for a, b in zip(again[:5], S[:5]):
            assert _same(a, b)
        for a, b in zip(again.sorted, S.sorted):
            assert _same(a, b)
        torch.cuda.synchronize()
        assert _plan_arrays(again.plan)["bad"] == 0
    GraphPlan.clear_cache()


# ------------------------------------------------------------------ 2. forward
FWD_SHAPES = [(16, 12, 3), (24, 10, 3), (8, 18, 2)]          # 160, 144 and 152 nodes


def _regular_pieces(schema, feat_dim, seed):
    return [synthetic_sampled_batch(schema, n_seed=s, width=w, depth=d, feat_dim=feat_dim, seed=seed + i)
            for i, (s, w, d) in enumerate(FWD_SHAPES)]


def _cpu(g):
    return [None if t is None else t.cpu() for t in g[:5]]


@pytest.mark.parametrize("use_RTE", [True, False])
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_layer_on_stacked_pieces_matches_fp64_and_the_pieces_alone(precision, use_RTE):
    d, H = 64, 4
    GraphPlan.clear_cache()
    parts = [to_device_graph(*p, device=DEV) for p in _regular_pieces("mag", d, 60)]
    S = stack_device_graphs(parts)
    T, R = len(S[5]), len(S[6])
    assert [g[1].numel() for g in parts] == [160, 144, 152]
    sd = O.make_state_dict(d, d, T, R, H, True, use_RTE, seed=5)
    layer = HGTConv(d, d, T, R, H, 0.2, True, use_RTE, precision=precision).eval()
    layer.load_state_dict(sd)
    layer = layer.to(DEV)
    x, nt, tm, ei, et = _cpu(S)
    ref = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, use_norm=True, use_RTE=use_RTE, dtype=torch.float64).to(DEV)
    gate = PREC_TOL[precision]
    with torch.no_grad():
        out = layer(S[0], S[1], S[3], S[4], S[2])
        alone = [layer(g[0], g[1], g[3], g[4], g[2]) for g in parts]
    err = (out.double() - ref).abs().max().item()
    errs_alone, diffs = [], []
    for got, one, want in zip(S.unstack(out), alone, S.unstack(ref)):
        errs_alone.append((one.double() - want).abs().max().item())
        diffs.append((got - one).abs().max().item())
    print("stacked %s RTE=%s: max|err| %.2e, pieces alone %s, stacked - alone %s (gate %.0e)"
          % (precision, use_RTE, err, ["%.1e" % e for e in errs_alone], ["%.1e" % e for e in diffs], gate))
    assert err < gate and max(errs_alone) < gate
    assert max(diffs) < 2 * gate
    GraphPlan.clear_cache()


def _gnn_fp64(P, g, T, R, H, n_layers, d):
    """pyhgt_amd.GNN in float64 torch on the CPU from the parameter dictionary P (adapter + tanh, then the closed-form layers)."""
    x, nt, tm, ei, et = g
    h = torch.zeros(x.size(0), d, dtype=torch.float64)
    for t in range(T):
        idx = (nt == t).nonzero().flatten()
        h = h.index_add(0, idx, torch.tanh(x[idx].double() @ P["adapt_ws.%d.weight" % t].T + P["adapt_ws.%d.bias" % t]))
    for li in range(n_layers):
        pre = "gcs.%d.base_conv." % li
        sd = {k[len(pre):]: v for k, v in P.items() if k.startswith(pre)}
        h = O.forward_closed_form(sd, T, R, H, h, nt, ei, et, tm, use_norm=True, use_RTE=True)
    return h


def test_two_layer_gnn_on_stacked_pieces():
    in_dim, d, H = 48, 64, 4
    GraphPlan.clear_cache()
    parts = [to_device_graph(*p, device=DEV) for p in _regular_pieces("oag", in_dim, 70)]
    S = stack_device_graphs(parts)
    T, R = len(S[5]), len(S[6])
    torch.manual_seed(2)
    gnn = GNN(in_dim, d, T, R, H, 2, prev_norm=True, last_norm=True, use_RTE=True).eval()
    P = {k: v.detach().clone().double() for k, v in gnn.state_dict().items()}
    with torch.no_grad():
        ref = _gnn_fp64(P, _cpu(S), T, R, H, 2, d).to(DEV)
    gnn = gnn.to(DEV)
    with torch.no_grad():
        out = gnn(S[0], S[1], S[2], S[3], S[4])
        alone = [gnn(g[0], g[1], g[2], g[3], g[4]) for g in parts]
    gate = 2e-4                                     # two layers (tests/test_hgt_gpu.py, the hand-off test)
    err = (out.double() - ref).abs().max().item()
    errs_alone = [(one.double() - want).abs().max().item() for one, want in zip(alone, S.unstack(ref))]
    diffs = [(got - one).abs().max().item() for got, one in zip(S.unstack(out), alone)]
    print("stacked 2-layer GNN: max|err| %.2e, pieces alone %s, stacked - alone %s" % (err, errs_alone, diffs))
    assert err < gate and max(errs_alone) < gate and max(diffs) < 2 * gate
    GraphPlan.clear_cache()


# ------------------------------------------------------------------ 3. across the route lines
def test_six_c3_pieces_cross_the_route_lines():
    """Six pieces of 3 200 nodes (each below the 4 608-target line) stack to 19 200 (above the 16 384-target fused line): 256 seeded
    rows against the fp64 closed form on their induced in-neighbourhood, both precisions."""
    d, H = 256, 8
    GraphPlan.clear_cache()
    parts = [to_device_graph(*synthetic_sampled_batch("mag", n_seed=128, width=128, depth=6, feat_dim=d, mean_degree=4.0, seed=30 + i),
                             device=DEV, plan=False) for i in range(6)]
    assert all(g[1].numel() == 3200 for g in parts)
    S = stack_device_graphs(parts)
    x, nt, tm, ei, et = S[:5]
    N, T, R = nt.numel(), len(S[5]), len(S[6])
    assert N == 19200 and N > 16384 and 3200 < 4608
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=77)
    gen = torch.Generator().manual_seed(9)
    tg = torch.sort(torch.randperm(N, generator=gen)[:256]).values.to(DEV)
    g = dict(T=T, R=R, H=H, d=d, ids=torch.arange(N, device=DEV).unsqueeze(1), nt=nt, ei=ei, et=et, tm=tm, use_rte=True, use_norm=True,
             deg=torch.bincount(ei[1], minlength=N), x=x)
    ref = _fp64_rows(sd, g, tg)
    for precision in ("f16x3", "bf16x3"):
        layer = HGTConv(d, d, T, R, H, 0.2, True, True, precision=precision).eval()
        layer.load_state_dict(sd)
        layer = layer.to(DEV)
        with torch.no_grad():
            out = layer(x, nt, ei, et, tm)
        err = (out[tg].double() - ref).abs().max().item()
        print("6 x c3 stacked, N=%d E=%d %s: max|err| on 256 rows %.2e (gate %.0e)" % (N, et.numel(), precision, err, PREC_TOL[precision]))
        assert bool(torch.isfinite(out).all()) and err < PREC_TOL[precision]
    GraphPlan.clear_cache()


# ------------------------------------------------------------------ 4. training
def _close(name, got, ref, factor=1.0):
    """BG._grads_close with every bound times `factor`."""
    ref = ref.detach().cpu().to(torch.float64)
    got = got.detach().cpu().to(torch.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(ref.abs().max().item(), 1e-12)
    diff = (got - ref).abs()
    err = diff.max().item() / scale
    assert err < factor * 5e-4, "%s: max |grad - reference| = %.3e of the largest entry (%.3e)" % (name, err, scale)
    rms = max(ref.pow(2).mean().sqrt().item(), 1e-12)
    excess = (diff - factor * (BG.ENTRY_ATOL * rms + BG.ENTRY_RTOL * ref.abs())).max().item()
    assert excess <= 0.0, "%s: an entry misses %g x (atol %.0e * rms + rtol %.0e) by %.3e" % (name, factor, BG.ENTRY_ATOL, BG.ENTRY_RTOL,
                                                                                              excess)
    return err


def _train_step(gnn, head, graph, rows, ys):
    """One forward + backward of the NLL loss summed over `rows` / `ys` (one entry per piece) -> (loss, parameter gradients,
    gradient of node_feature)."""
    for p in list(gnn.parameters()) + list(head.parameters()):
        p.grad = None
    x = graph[0].detach().clone().requires_grad_(True)
    rep = gnn(x, graph[1], graph[2], graph[3], graph[4])
    loss = sum(torch.nn.functional.nll_loss(head(rep[r]), y) for r, y in zip(rows, ys))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().clone() for k, v in list(gnn.named_parameters()) + [("head." + k, v) for k, v in head.named_parameters()]
             if v.grad is not None}
    return loss.item(), grads, x.grad.detach().clone()


@pytest.mark.parametrize("deterministic", [False, True])
def test_training_step_on_stacked_pieces(deterministic):
    """2-layer GNN (n_hid 64, 4 heads, dropout 0) + Classifier on the stacked seeds: every gradient against the fp64 backward of the
    stacked graph at the gates of tests/test_backward_gpu.py (its GNN step), within twice those gates of the sum of the three
    separate steps' gradients; deterministic=True: two stacked steps are bit-identical."""
    in_dim, d, H, n_cls = 16, 64, 4, 5
    GraphPlan.clear_cache()
    was = GraphPlan.CACHE_SIZE
    GraphPlan.CACHE_SIZE = 8
    try:
        parts = [to_device_graph(*p, device=DEV) for p in _regular_pieces("mag", in_dim, 80)]
        S = stack_device_graphs(parts)
        T, R = len(S[5]), len(S[6])
        n_seed = [s for s, _, _ in FWD_SHAPES]
        torch.manual_seed(1)
        gnn = GNN(in_dim, d, T, R, H, 2, dropout=0.0, prev_norm=True, last_norm=True, use_RTE=True, deterministic=deterministic).to(DEV).train()
        head = Classifier(d, n_cls, deterministic=deterministic).to(DEV).train()
        ys = [torch.randint(0, n_cls, (n,)) for n in n_seed]
        ys_dev = [y.to(DEV) for y in ys]
        rows = [S.rows(b, "paper", torch.arange(n)) for b, n in enumerate(n_seed)]
        loss, grads, xgrad = _train_step(gnn, head, S, rows, ys_dev)
        if deterministic:
            loss2, grads2, xgrad2 = _train_step(gnn, head, S, rows, ys_dev)
            assert loss == loss2 and torch.equal(xgrad, xgrad2) and grads.keys() == grads2.keys()
            for k in grads:
                assert torch.equal(grads[k], grads2[k]), k
        # fp64 backward of the stacked graph
        P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in list(gnn.named_parameters()) + [("head." + k, v) for k, v in
                                                                                                         head.named_parameters()]}
        xs, nt, tm, ei, et = _cpu(S)
        x64 = xs.double().requires_grad_(True)
        h = _gnn_fp64(P, (x64, nt, tm, ei, et), T, R, H, 2, d)
        ref_loss = sum(torch.nn.functional.nll_loss(torch.log_softmax(h[r.cpu()] @ P["head.linear.weight"].T + P["head.linear.bias"], dim=-1), y)
                       for r, y in zip(rows, ys))
        ref_loss.backward()
        assert abs(loss - ref_loss.item()) < 3e-4            # (1e-4 per summed piece loss, tests/test_backward_gpu.py)
        worst = 0.0
        for k, v in grads.items():
            if P[k].grad is not None:
                worst = max(worst, _close(k, v, P[k].grad))
        worst = max(worst, _close("node_feature", xgrad, x64.grad))
        # the three separate steps
        total, xparts, loss_sum = {}, [], 0.0
        for b, g in enumerate(parts):
            lb, gb, xb = _train_step(gnn, head, g, [torch.arange(n_seed[b], device=DEV) + g[5]["paper"][0]], [ys_dev[b]])
            loss_sum += lb
            xparts.append(xb)
            for k, v in gb.items():
                total[k] = total.get(k, 0) + v.double()
        assert abs(loss - loss_sum) < 6e-4 and grads.keys() == total.keys()
        worst2 = 0.0
        for k, v in grads.items():
            worst2 = max(worst2, _close(k + " (sum of the separate steps)", v, total[k], factor=2.0))
        for b, (got, one) in enumerate(zip(S.unstack(xgrad), xparts)):
            worst2 = max(worst2, _close("node_feature of piece %d (its separate step)" % b, got, one, factor=2.0))
        print("stacked training step (deterministic=%s): worst relative error vs fp64 %.2e, vs the separate steps %.2e"
              % (deterministic, worst, worst2))
    finally:
        GraphPlan.CACHE_SIZE = was
        GraphPlan.clear_cache()


# ------------------------------------------------------------------ 5. a piece that is not sorted
@pytest.mark.parametrize("swap", ["inside-a-type", "across-types"])
def test_unsorted_piece_raises_index_error_on_the_next_forward(swap):
    """Two targets of one relation swapped in a piece's sorted form, every id in range: the stack is built (bounds-checked stores,
    the maps stay permutations), the next forward raises the IndexError of GraphPlan.from_sorted, and the process goes on."""
    pieces = SB.piece_set("mag", feat_dim=32)
    GraphPlan.clear_cache()
    parts = [to_device_graph(*p, device=DEV, plan=False) for p in pieces]
    good = parts[1]
    src, dst, tm, rel_ptr, type_off = [a.clone() for a in good.sorted]
    rp, d_host = rel_ptr.cpu().numpy(), dst.cpu().numpy()
    r = good[6]["self"]                               # the relation with targets of every type
    i, j = (int(rp[r]), int(rp[r]) + 2) if swap == "inside-a-type" else (int(rp[r]) + 1, int(rp[r + 1]) - 1)
    to = type_off.cpu().numpy()
    same_type = np.searchsorted(to, d_host[i], side="right") == np.searchsorted(to, d_host[j], side="right")
    assert d_host[i] < d_host[j] and same_type == (swap == "inside-a-type")
    dst[i], dst[j] = int(d_host[j]), int(d_host[i])
    broken = _DeviceGraph(tuple(good))
    broken.sorted = (src, dst, tm, rel_ptr, type_off)
    S = stack_device_graphs([parts[0], broken, parts[2]])
    torch.cuda.synchronize()
    N, E = S[1].numel(), S[4].numel()
    assert np.array_equal(np.sort(S.node_map.cpu().numpy()), np.arange(N)) and np.array_equal(np.sort(S.edge_map.cpu().numpy()), np.arange(E))
    assert int(S.sorted[0].min()) >= 0 and int(S.sorted[0].max()) < N and int(S.sorted[1].min()) >= -1 and int(S.sorted[1].max()) < N
    T, R = len(S[5]), len(S[6])
    layer = HGTConv(32, 32, T, R, 4, 0.2, True, True, strict=True).eval().to(DEV)
    with pytest.raises(IndexError):
        with torch.no_grad():
            layer(S[0], S[1], S[3], S[4], S[2])
    torch.cuda.synchronize()
    _check_layout(pieces)                             # the process continues: a good stack right after
    GraphPlan.clear_cache()


# ------------------------------------------------------------------ 6. errors before any launch
def test_stack_rejects_what_cannot_be_stacked(monkeypatch):
    from pyhgt_amd import _lib
    GraphPlan.clear_cache()
    mag = [to_device_graph(*p, device=DEV, plan=False) for p in SB.piece_set("mag")]
    oag = to_device_graph(*SB.piece_set("oag")[1], device=DEV, plan=False)
    wide = to_device_graph(*synthetic_sampled_batch("mag", n_seed=4, width=4, depth=1, feat_dim=24, seed=1), device=DEV, plan=False)
    no_time = to_device_graph(*SB.without_time(SB.piece_set("mag"))[1], device=DEV, plan=False)
    other_rel = _DeviceGraph(tuple(mag[1][:6]) + (dict(mag[1][6], extra=len(mag[1][6])),))
    other_rel.sorted = mag[1].sorted
    lib = _lib.load()

    class NoLaunch:
        """The library with the two entry points that launch replaced: a ValueError must come before either is reached."""
        def __getattr__(self, name):
            if name in ("hgt_stack_sorted", "hgt_gather_rows", "hgt_plan_from_sorted"):
                raise AssertionError("%s reached" % name)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "_lib", NoLaunch())
    for bad in ([], [mag[0], oag], [mag[1], wide], [mag[1], no_time], [no_time, mag[1]], [mag[1], other_rel],
                [mag[1], tuple(mag[2])]):
        with pytest.raises(ValueError):
            stack_device_graphs(bad)
    with pytest.raises(AssertionError):
        stack_device_graphs(mag)                     # (the guard is live: a good call does reach the library)
    monkeypatch.undo()
    assert stack_device_graphs(mag).n_graphs == 3
    GraphPlan.clear_cache()


# ------------------------------------------------------------------ 7. the example loop
def test_training_loop_with_stacked_batches_reduces_the_loss():
    """examples/train_synthetic.py --stack 2: two sampled batches per optimizer step; the criterion of
    tests/test_backward_gpu.py::test_training_loop_reduces_the_loss."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(SB.ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.run("mag", steps=40, verbose=False, stack=2)
    assert all(l == l for l in losses)                              # finite
    assert sum(losses[-8:]) / 8 < 0.8 * sum(losses[:4]) / 4, (losses[:4], losses[-8:])
    GraphPlan.clear_cache()
