"""GPU tests of training with heads wider than 64 padded columns (n_hid 768 / 1024 with 8 heads, 512 with 4 or 2, 256 with 2 or 1,
400 with 4): the two primitives that carry the width -- hgt_relation_outer_wide (heads of 128 / 256 padded columns) and the
16-columns-per-lane instantiation of hgt_node_update_bwd[_ex] (rows of 513 .. 1024 columns) -- against their fp64 restatements
(oracle/backward_primitives.py), whole HGTConv / DenseHGTConv layers and a 2-layer GNN against oracle.backward_reference, and the
limit that stays (heads wider than 256 columns).  Helpers, graphs and tolerances are those of tests/test_backward_kernels_gpu.py
and tests/test_backward_gpu.py, imported from there."""
import ctypes as C

import pytest
import torch

import test_backward_gpu as BG
import test_backward_kernels_gpu as BK
from oracle import backward_primitives as BP
from oracle import hgt_oracle as O
from pyhgt_amd import HGTConv, DenseHGTConv, GNN, Classifier, GraphPlan, _lib
from pyhgt_amd.autograd import logits_form, outer_form, training_supported
from pyhgt_amd.synth import synthetic_typed_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HGT_ERR_UNSUPPORTED = -2
_st, _p, _close, _gen, _randn = BK._st, BK._p, BK._close, BK._gen, BK._randn
_grads_close = BG._grads_close


# ------------------------------------------------------------------------------------------------------------------------------
# hgt_relation_outer_wide
# ------------------------------------------------------------------------------------------------------------------------------
def wide_items_per_workgroup_factor(max_items):
    # mirrors outer_wide_items_per_wg (pyhgt_amd/csrc/hgt_bwd_outer.hip): 8 (R + 1) items per workgroup below 16 384 plan items, else
    # 64 (R + 1) -- four wavefronts x the 2 / 16 of outer_items_per_wave
    return 8 if max_items < 16384 else 64


WIDE_OUTER_CASES = [
    # name, d, H, T, R, N, E, rte, expected dk_pad, expected items-per-workgroup factor
    ("w128_d512h4_r1_small_rte", 512, 4, 3, 1, 3000, 24000, True, 128, 8),
    ("w128_d768h8_r8_small_plain", 768, 8, 3, 8, 4000, 30000, False, 128, 8),          # d_k 96, padded to 128
    ("w128_d1024h8_r33_large_rte", 1024, 8, 3, 33, 66000, 500000, True, 128, 64),
    ("w128_d768h8_r33_large_plain", 768, 8, 3, 33, 66000, 500000, False, 128, 64),
    ("w256_d512h2_r8_small_rte", 512, 2, 3, 8, 4000, 30000, True, 256, 8),
    ("w256_d768h4_r1_small_plain", 768, 4, 2, 1, 3000, 24000, False, 256, 8),          # d_k 192, padded to 256
    ("w256_d768h4_r33_large_rte", 768, 4, 3, 33, 66000, 500000, True, 256, 64),
    ("w256_d512h2_r33_large_plain", 512, 2, 3, 33, 70000, 500000, False, 256, 64),
]


def test_wide_outer_cases_cover_both_widths_regimes_and_rte():
    seen = {(c[8], c[9], c[7]) for c in WIDE_OUTER_CASES}                      # (dk_pad, items-per-workgroup factor, RTE)
    assert {(w, i, r) for w in (128, 256) for i in (8, 64) for r in (True, False)} <= seen
    assert {c[4] for c in WIDE_OUTER_CASES} >= {1, 8, 33}
    assert {(c[1], c[2]) for c in WIDE_OUTER_CASES} >= {(512, 4), (768, 8), (1024, 8), (512, 2), (768, 4)}


@pytest.mark.parametrize("case", WIDE_OUTER_CASES, ids=[c[0] for c in WIDE_OUTER_CASES])
def test_relation_outer_wide_matches_fp64(case):
    name, d, H, T, R, N, E, rte, dkp_exp, ipw = case
    lib = _lib.load()
    lay = BK._layout(d, H)
    assert lay.dk_pad == dkp_exp, "the head-padded layout moved: re-aim %s" % name
    assert wide_items_per_workgroup_factor(BK._max_items(N, E, T, R)) == ipw, "the items-per-workgroup threshold moved: re-aim %s" % name
    Hl, dkp, dp = lay.heads, lay.dk_pad, lay.d_pad
    nt, ei, et, tm = BK._graph(N, E, T, R, seed=N + R + d, rte=rte, empty_rel=min(1, R - 1) if R > 1 else None)
    plan = GraphPlan(nt, ei, et, tm, T, R)
    g = _gen(d + H)
    w_id = _randn((E, Hl), g)
    a = _randn((N, dp), g)
    b = _randn((N, dp), g)
    rte_a = _randn((T * 240, dp), g) if rte else None
    out0 = torch.randn(R, Hl, dkp, dkp, generator=g, device=DEV)            # the call accumulates
    out = out0.clone()
    w = BK._to_sorted(plan, w_id, T, R)                                      # weights by edge id -> plan order
    assert lib.hgt_relation_outer_wide(plan.ptr, N, E, T, R, Hl, dkp, w.data_ptr(), a.data_ptr(), _p(rte_a), b.data_ptr(), out.data_ptr(),
                                       _st()) == 0
    torch.cuda.synchronize()
    src, dst, rel, rrow = BP.plan_edges(nt, ei, et, tm, T, R)
    ref = BP.relation_outer(src, dst, rel, rrow, w_id, a, rte_a, b, R, Hl, dkp)
    got = out.double() - out0.double()
    if R > 1:
        assert bool((rel == 1).sum() == 0) and torch.equal(out[1], out0[1]), "a relation without edges must stay untouched"
    err = _close("relation_outer_wide", got, ref, 2e-5, 1e-4)
    print("relation_outer_wide %s: max |kernel - fp64| = %.2e of the largest entry" % (name, err))


@pytest.mark.parametrize("d,H,dkp", [(256, 4, 64), (512, 1, 512)])
def test_relation_outer_wide_rejects_other_widths(d, H, dkp):
    lib = _lib.load()
    T, R, N, E = 2, 3, 500, 3000
    lay = BK._layout(d, H)
    assert lay.dk_pad == dkp
    nt, ei, et, _ = BK._graph(N, E, T, R, seed=3, rte=False)
    plan = GraphPlan(nt, ei, et, None, T, R)
    w = torch.ones(E, lay.heads, device=DEV)
    a = torch.ones(N, lay.d_pad, device=DEV)
    out = torch.full((R, lay.heads, dkp, dkp), 3.0, device=DEV)
    assert lib.hgt_relation_outer_wide(plan.ptr, N, E, T, R, lay.heads, dkp, w.data_ptr(), a.data_ptr(), 0, a.data_ptr(), out.data_ptr(),
                                       _st()) == HGT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# hgt_node_update_bwd / hgt_node_update_bwd_ex on rows of 513 .. 1024 columns
# ------------------------------------------------------------------------------------------------------------------------------
WIDE_NUB_DIMS = [576, 768, 1000, 1024]        # 576: the first width past 512; 1000: the last 64-column group is partial; 1024 = 16 * 64
WIDE_NUB_ROWS = [(3001, 2), (16384, 8), (65536, 32)]
WIDE_NUB_CASES = []
for _i, (_n, _rpw) in enumerate(WIDE_NUB_ROWS):
    for _j, _form in enumerate(BK.NUB_FORMS):
        for _m in (False, True):
            WIDE_NUB_CASES.append((_n, _rpw, _form, WIDE_NUB_DIMS[(_i + _j + 2 * _m) % 4], BK.NUB_TYPES[(_i + 2 * _j + _m) % 3], _m))


def test_wide_node_update_cases_cover_every_branch_form_and_width():
    assert {BK.nub_rows_per_wave(n) for n, *_ in WIDE_NUB_CASES} == {2, 8, 32}
    for rpw in (2, 8, 32):
        assert {(c[2], c[5]) for c in WIDE_NUB_CASES if c[1] == rpw} == {(f, m) for f in BK.NUB_FORMS for m in (False, True)}
    assert {c[3] for c in WIDE_NUB_CASES} == set(WIDE_NUB_DIMS)
    assert all(512 < c[3] <= 1024 for c in WIDE_NUB_CASES)


@pytest.mark.parametrize("n,rpw,form,d,types,masked", WIDE_NUB_CASES,
                         ids=["%d-%s-d%d-%s%s" % (c[0], c[2], c[3], c[4], "-mask" if c[5] else "") for c in WIDE_NUB_CASES])
def test_node_update_bwd_wide_rows_match_fp64(n, rpw, form, d, types, masked):
    assert BK.nub_rows_per_wave(n) == rpw, "the rows-per-wavefront thresholds moved: re-aim this case"
    lib = _lib.load()
    T = 3
    g = _gen(n + d)
    gated = form.startswith("gated")
    use_norm = form != "gated_plain"
    shared = form == "residual_shared_norm"
    nt = BK._node_types(n, T, types, g)
    ldx, ld_dx = d + 12, d + 20
    trans = _randn((n, d), g)
    xbuf = _randn((n, ldx), g)
    gout = _randn((n, d), g)
    skip = torch.randn(T, generator=g, device=DEV) if gated else None
    ln_w = (1.0 + 0.2 * torch.randn(T, d, generator=g, device=DEV)) if use_norm else None
    mask = (torch.bernoulli(torch.full((n, d), 0.8, device=DEV), generator=g) / 0.8) if masked else None
    if mask is not None:
        trans = trans * mask
    d_trans = torch.full((n, d), 7.0, device=DEV)
    dx = torch.full((n, ld_dx), -9.0, device=DEV)
    d_alpha0 = torch.randn(T, generator=g, device=DEV)
    d_lnw0 = torch.randn(T, d, generator=g, device=DEV)
    d_lnb0 = torch.randn(T, d, generator=g, device=DEV)
    d_alpha, d_lnw, d_lnb = d_alpha0.clone(), d_lnw0.clone(), d_lnb0.clone()
    args_tail = (_p(mask), n, d, T, _p(d_trans), _p(dx), ld_dx, _p(d_alpha) if gated else 0, _p(d_lnw) if use_norm else 0,
                 _p(d_lnb) if use_norm else 0, _st())
    if gated:
        rc = lib.hgt_node_update_bwd(_p(gout), _p(trans), _p(xbuf), ldx, _p(nt), _p(skip), _p(ln_w), int(use_norm), *args_tail)
    else:
        rc = lib.hgt_node_update_bwd_ex(_p(gout), _p(trans), _p(xbuf), ldx, _p(nt), _p(skip), _p(ln_w), int(use_norm), int(shared),
                                        *args_tail)
    assert rc == 0
    torch.cuda.synchronize()
    ref = BP.node_update_bwd(gout, trans, xbuf, nt, T, skip=skip, ln_w=ln_w, use_norm=use_norm, shared_norm=shared, drop_mask=mask)
    unknown = (nt < 0) | (nt >= T)
    assert bool((d_trans[unknown] == 0).all()) and bool((dx[unknown, :d] == 0).all()), "rows of unknown type must be exact zeros"
    assert bool((dx[:, d:] == -9.0).all()), "dx written beyond d columns"
    _close("d_trans", d_trans, ref["d_trans"], 1e-5, 1e-4)
    _close("dx", dx[:, :d], ref["dx"], 1e-5, 1e-4)
    if gated:
        _close("d_alpha", d_alpha.double() - d_alpha0.double(), ref["d_alpha"], 1e-4, 1e-4)
    if use_norm:
        rows = 1 if shared else T
        _close("d_ln_w", d_lnw[:rows].double() - d_lnw0[:rows].double(), ref["d_ln_w"], 1e-4, 1e-4)
        _close("d_ln_b", d_lnb[:rows].double() - d_lnb0[:rows].double(), ref["d_ln_b"], 1e-4, 1e-4)
        if shared:
            assert torch.equal(d_lnw[1:], d_lnw0[1:]) and torch.equal(d_lnb[1:], d_lnb0[1:]), "shared norm wrote past row 0"


# ------------------------------------------------------------------------------------------------------------------------------
# whole layers
# ------------------------------------------------------------------------------------------------------------------------------
WIDE_CASES = [
    # name, T, R, H, d, N, E, use_norm, use_RTE, graph kwargs, tweaks
    ("d256_h2", 3, 4, 2, 256, 1200, 8000, True, False, {}, {}),                                       # dk_pad 128
    ("d512_h4_hubs", 3, 5, 4, 512, 1500, 9000, True, False, dict(dst_skew=1.1), dict(hub=True, unclaimed=True)),
    ("d400_h4_unsorted", 2, 3, 4, 400, 1500, 9000, True, True, dict(sorted_types=False), dict(unknown=True)),     # d_k 100 -> 128
    ("d768_h8_rte", 3, 4, 8, 768, 1000, 6000, True, True, {}, {}),                                    # d_k 96 -> 128, rows of 1024
    ("d1024_h8", 3, 4, 8, 1024, 1000, 6000, True, False, {}, {}),
    ("d768_h4_rte", 2, 3, 4, 768, 1200, 7000, True, True, {}, {}),                                    # d_k 192 -> 256
    ("d256_h1", 2, 2, 1, 256, 1000, 6000, True, True, {}, {}),                                        # dk_pad 256, one head
]
WIDE_DENSE_CASES = [
    ("dense_d512_h4", 3, 4, 4, 512, 1200, 8000, True, False, {}, dict(unknown=True, unclaimed=True)),
    ("dense_d768_h4_rte", 2, 3, 4, 768, 1000, 6000, True, True, {}, {}),
]


def test_wide_layer_cases_are_wide_and_supported():
    for c in WIDE_CASES + WIDE_DENSE_CASES:
        lay = _lib.layout_for(c[4], c[3])
        assert lay.dk_pad in (128, 256), c[0]
        assert logits_form(lay.dk_pad) == "mfma" and outer_form(lay.dk_pad) == "hgt_relation_outer_wide", c[0]
        assert training_supported(c[4], c[3])[0], c[0]
    assert {(c[4], c[3]) for c in WIDE_CASES} == {(256, 2), (512, 4), (400, 4), (768, 8), (1024, 8), (768, 4), (256, 1)}
    assert {(c[4], c[3]) for c in WIDE_DENSE_CASES} == {(512, 4), (768, 4)}


def _tweaked_graph(N, E, d, T, R, seed, gk, tw):
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=seed, **gk)
    nt, et, ei = nt.clone(), et.clone(), ei.clone()
    if tw.get("unknown"):
        nt[::13] = T + 1                    # nodes no typed layer claims
    if tw.get("unclaimed"):
        et[::7] = R                         # edges no meta relation claims
    if tw.get("hub"):
        ei[1, :4000] = 17                   # > 1024 in-edges: a hub of the plan ...
        ei[0, 4000:7000] = 23               # ... and > 1024 out-edges: a hub of the transposed plan
    return x, nt, ei, et, tm


def _layer_backward_check(cls, case, precision, dense):
    name, T, R, H, d, N, E, use_norm, use_RTE, gk, tw = case
    sd = O.make_state_dict(d, d, T, R, H, use_norm, use_RTE, seed=11, dense=dense)
    x, nt, ei, et, tm = _tweaked_graph(N, E, d, T, R, 12, gk, tw)
    if tw.get("hub"):
        assert torch.bincount(ei[1], minlength=N).max().item() > 1024 and torch.bincount(ei[0], minlength=N).max().item() > 1024
    gout = torch.randn(N, d, generator=torch.Generator().manual_seed(5))
    tme = tm if use_RTE else None
    ref = O.backward_reference(sd, T, R, H, x, nt, ei, et, tme, gout, use_norm=use_norm, use_RTE=use_RTE, dense=dense)
    layer = cls(d, d, T, R, H, 0.2, use_norm, use_RTE, precision=precision).eval()
    layer.load_state_dict(sd)
    layer = layer.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    GraphPlan.clear_cache()
    out = layer(xd, nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV) if use_RTE else None)
    fwd = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tme, use_norm=use_norm, use_RTE=use_RTE, dense=dense)
    ferr = (out.detach().cpu().double() - fwd).abs().max().item()
    print("wide %s / %s: forward max |out - fp64| = %.2e" % (name, precision, ferr))
    assert ferr < 1e-4
    out.backward(gout.to(DEV))
    torch.cuda.synchronize()
    errs = {"x": (xd.grad, ref["x"])}
    for k, p in layer.named_parameters():
        if k == "emb.emb.weight" and p.grad is None:
            continue
        assert p.grad is not None, k
        errs[k] = (p.grad, ref[k])
    for k, (got, r) in errs.items():      # every figure first, then the assertions
        r64 = r.to(torch.float64)
        print("wide %s / %s: %-28s max err %.2e of the largest entry (%.2e)" % (
            name, precision, k, (got.detach().cpu().double() - r64).abs().max().item() / max(r64.abs().max().item(), 1e-12),
            r64.abs().max().item()))
    worst = max(_grads_close(k, got, r) for k, (got, r) in errs.items())
    print("wide backward %s / %s: worst relative gradient error %.2e over %d tensors" % (name, precision, worst, len(errs)))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "f16x3"])
@pytest.mark.parametrize("case", WIDE_CASES, ids=[c[0] for c in WIDE_CASES])
def test_wide_hgtconv_backward_matches_oracle(case, precision):
    _layer_backward_check(HGTConv, case, precision, dense=False)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "f16x3"])
@pytest.mark.parametrize("case", WIDE_DENSE_CASES, ids=[c[0] for c in WIDE_DENSE_CASES])
def test_wide_dense_hgtconv_backward_matches_oracle(case, precision):
    _layer_backward_check(DenseHGTConv, case, precision, dense=True)


@pytest.mark.parametrize("conv,d,H", [("hgt", 768, 8), ("dense", 512, 4)])
def test_wide_dropout_gradients_match_the_oracle_with_the_drawn_masks(conv, d, H, monkeypatch):
    """Training mode at a wide layout: the masks the forward draws are captured at torch.bernoulli and replayed in the oracle
    (the manner of test_dropout_gradients_match_the_oracle_with_the_drawn_masks)."""
    dense = conv == "dense"
    T, R, N, E, p = 3, 4, 1200, 8000, 0.2
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=51, dense=dense)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=52, sorted_types=False)
    nt = nt.clone()
    nt[::17] = T + 1
    layer = (DenseHGTConv if dense else HGTConv)(d, d, T, R, H, p, True, True, keep_att=True)
    layer.load_state_dict(sd)
    layer = layer.to(DEV).train()
    drawn = []
    real_bernoulli = torch.bernoulli

    def recording_bernoulli(*a, **k):
        out = real_bernoulli(*a, **k)
        drawn.append(out.clone())
        return out

    monkeypatch.setattr(torch, "bernoulli", recording_bernoulli)
    gout = torch.randn(N, d, generator=torch.Generator().manual_seed(53))
    xd = x.to(DEV).requires_grad_(True)
    GraphPlan.clear_cache()
    out = layer(xd, nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV))
    out.backward(gout.to(DEV))
    torch.cuda.synchronize()
    monkeypatch.undo()
    n_masks = 2 if dense else 1
    assert len(drawn) == n_masks
    masks = [(m / (1.0 - p)).cpu() for m in drawn]
    assert all(0.75 < float((m != 0).float().mean()) < 0.85 for m in masks)
    dm = (masks[0], masks[1] if dense else None)
    fwd, att = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, use_norm=True, dense=dense, drop_masks=dm, return_att=True)
    assert (out.detach().cpu().double() - fwd).abs().max().item() < 1e-4
    assert layer.att is not None and (layer.att.cpu().double() - att).abs().max().item() < 1e-5
    ref = O.backward_reference(sd, T, R, H, x, nt, ei, et, tm, gout, use_norm=True, dense=dense, drop_masks=dm)
    worst = _grads_close("x", xd.grad, ref["x"])
    for k, prm in layer.named_parameters():
        if k == "emb.emb.weight" and prm.grad is None:
            continue
        assert prm.grad is not None, k
        worst = max(worst, _grads_close(k, prm.grad, ref[k]))
    print("wide dropout %s d=%d: worst relative gradient error %.2e" % (conv, d, worst))


# ------------------------------------------------------------------------------------------------------------------------------
# a model
# ------------------------------------------------------------------------------------------------------------------------------
def test_wide_gnn_training_step_matches_autograd_through_the_oracle():
    """test_gnn_training_step_matches_autograd_through_the_oracle at n_hid 768 / 8 heads (heads of 96 -> 128 padded columns)."""
    T, R, H, in_dim, d, N, E, n_cls = 3, 4, 8, 37, 768, 1200, 8000, 5
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, in_dim, T, R, seed=21)
    torch.manual_seed(1)
    gnn = GNN(in_dim, d, T, R, H, 2, dropout=0.0, prev_norm=True, last_norm=True, use_RTE=True).to(DEV).train()
    head = Classifier(d, n_cls).to(DEV).train()
    y = torch.randint(0, n_cls, (200,))
    rep = gnn(x.to(DEV), nt.to(DEV), tm.to(DEV), ei.to(DEV), et.to(DEV))
    loss = torch.nn.functional.nll_loss(head(rep[:200]), y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    named = list(gnn.named_parameters()) + [("head." + k, v) for k, v in head.named_parameters()]
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in named}
    h = torch.zeros(N, d, dtype=torch.float64)
    for t in range(T):
        idx = (nt == t).nonzero().flatten()
        h = h.index_add(0, idx, torch.tanh(x[idx].double() @ P["adapt_ws.%d.weight" % t].T + P["adapt_ws.%d.bias" % t]))
    for li in range(2):
        sd = {k[len("gcs.%d.base_conv." % li):]: v for k, v in P.items() if k.startswith("gcs.%d.base_conv." % li)}
        h = O.forward_closed_form(sd, T, R, H, h, nt, ei, et, tm, use_norm=True, use_RTE=True)
    logp = torch.log_softmax(h[:200] @ P["head.linear.weight"].T + P["head.linear.bias"], dim=-1)
    ref_loss = torch.nn.functional.nll_loss(logp, y)
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-4
    worst = 0.0
    for k, v in named:
        if P[k].grad is None:
            continue
        worst = max(worst, _grads_close(k, v.grad, P[k].grad, rtol=5e-4))
    print("wide GNN training step: worst relative gradient error %.2e" % worst)


def test_wide_training_loop_reduces_the_loss():
    """examples/train_synthetic.py at n_hid 768 / 8 heads: the loss of a short loop on a learnable synthetic task falls."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.run("mag", steps=40, conv="hgt", n_hid=768, n_heads=8, verbose=False)
    assert all(l == l for l in losses)                              # finite
    assert sum(losses[-8:]) / 8 < 0.8 * sum(losses[:4]) / 4, (losses[:4], losses[-8:])


# ------------------------------------------------------------------------------------------------------------------------------
# the limit that stays: heads wider than 256 padded columns
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", [(512, 1), (1024, 2)])
def test_heads_wider_than_256_columns_train_nowhere_and_still_infer(d, H, monkeypatch):
    T, R, N, E = 2, 3, 600, 4000
    ok, reason = training_supported(d, H)
    assert not ok and "256" in reason
    sd = O.make_state_dict(d, d, T, R, H, True, False, seed=3)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=4)
    layer = HGTConv(d, d, T, R, H, 0.2, True, False)
    layer.load_state_dict(sd)
    layer = layer.to(DEV).train()
    args = [x.to(DEV), nt.to(DEV), ei.to(DEV), et.to(DEV), None]
    # before ANY C call of the training path: for the duration of the raises block every entry of the loaded library raises, except
    # what runs ahead of hgt_conv_train's guard -- the plan (hgt_plan_*), the layout arithmetic, error strings
    real = _lib.load()

    class NoKernel:
        def __getattr__(self, name):
            if name.startswith("hgt_plan_") or name in ("hgt_layout_for", "hgt_strerror"):
                return getattr(real, name)
            raise AssertionError("%s was reached before the limit was stated" % name)

    monkeypatch.setattr(_lib, "_lib", NoKernel())
    with pytest.raises(NotImplementedError, match="at most 256"):
        layer(*args)
    monkeypatch.undo()
    layer.eval()
    with torch.no_grad():
        out = layer(*args)
    torch.cuda.synchronize()
    ref = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, None, use_norm=True, use_RTE=False)
    assert (out.cpu().double() - ref).abs().max().item() < 1e-4
