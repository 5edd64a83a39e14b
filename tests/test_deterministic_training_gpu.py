"""GPU tests of the bit-reproducible training mode (deterministic=True): every `_det` entry point against its float64 restatement
(oracle/backward_primitives.py) with the tolerances of the atomic forms (tests/test_backward_kernels_gpu.py, test_backward_gpu.py)
and bit-equal across two calls; whole layers, a GNN training loop and the guards.  Each case runs its step twice: a comparison, not
a hunt for a rare event -- and nothing here asserts that the default path differs between runs (it may coincide)."""
import ctypes as C

import pytest
import torch

import test_backward_gpu as BG
import test_backward_kernels_gpu as BK
from oracle import backward_primitives as BP
from oracle import hgt_oracle as O
import pyhgt_amd
from pyhgt_amd import HGTConv, DenseHGTConv, GNN, Classifier, GraphPlan, _lib
from pyhgt_amd.autograd import TENSOR_SLOTS, spmm_takes_items, training_supported
from pyhgt_amd.synth import synthetic_typed_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_st, _p, _close, _gen, _randn = BK._st, BK._p, BK._close, BK._gen, BK._randn
_grads_close = BG._grads_close


def _ws(name, *args):
    nb = C.c_uint64()
    assert getattr(_lib.load(), name + "_bytes")(*args, C.byref(nb)) == 0
    return torch.empty(max(int(nb.value), 16), dtype=torch.uint8, device=DEV), int(nb.value)


# ------------------------------------------------------------------------------------------------------------------------------
# per entry point
# ------------------------------------------------------------------------------------------------------------------------------
NUB_DET_CASES = [
    # rows, form, d, node-type pattern, dropout mask        (slots: rows / 4 up to 4096 wavefronts)
    (9, "gated_norm", 64, "shuffled", False),                # a handful of slots
    (3001, "gated_norm", 256, "runs7", True),
    (40000, "gated_plain", 400, "shuffled", False),          # 4096 slots: the two-pass reduce
    (70001, "residual_shared_norm", 512, "runs33", True),
    (16384, "gated_norm", 768, "shuffled", True),            # rows past 512 columns: the 16-columns-per-lane instantiation
    (5000, "residual_norm", 1000, "runs7", False),
]


@pytest.mark.parametrize("n,form,d,types,masked", NUB_DET_CASES, ids=["%d-%s-d%d" % c[:3] for c in NUB_DET_CASES])
def test_node_update_bwd_det(n, form, d, types, masked):
    lib = _lib.load()
    T = 4                                                      # type 3 never occurs: a type with zero rows
    g = _gen(n + d)
    gated, use_norm, shared = form.startswith("gated"), form != "gated_plain", form == "residual_shared_norm"
    nt = BK._node_types(n, 3, types, g)
    ldx = d + 12
    trans, xbuf, gout = _randn((n, d), g), _randn((n, ldx), g), _randn((n, d), g)
    skip = torch.randn(T, generator=g, device=DEV) if gated else None
    ln_w = (1.0 + 0.2 * torch.randn(T, d, generator=g, device=DEV)) if use_norm else None
    mask = (torch.bernoulli(torch.full((n, d), 0.8, device=DEV), generator=g) / 0.8) if masked else None
    if mask is not None:
        trans = trans * mask
    ws, nb = _ws("hgt_node_update_bwd_det", n, d, T)
    runs = []
    for _ in range(2):
        d_trans, dx = torch.full((n, d), 7.0, device=DEV), torch.full((n, ldx), -9.0, device=DEV)
        # the outputs are OVERWRITTEN: sentinels must vanish
        d_alpha, d_lnw, d_lnb = (torch.full(s, 3.0, device=DEV) for s in ((T,), (T, d), (T, d)))
        assert lib.hgt_node_update_bwd_det(_p(gout), _p(trans), _p(xbuf), ldx, _p(nt), _p(skip), _p(ln_w), int(use_norm), int(shared),
                                           _p(mask), n, d, T, _p(d_trans), _p(dx), ldx, _p(d_alpha) if gated else 0,
                                           _p(d_lnw) if use_norm else 0, _p(d_lnb) if use_norm else 0, ws.data_ptr(), nb, _st()) == 0
        torch.cuda.synchronize()
        runs.append((d_trans, dx, d_alpha, d_lnw, d_lnb))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    d_trans, dx, d_alpha, d_lnw, d_lnb = runs[0]
    ref = BP.node_update_bwd(gout, trans, xbuf, nt, T, skip=skip, ln_w=ln_w, use_norm=use_norm, shared_norm=shared, drop_mask=mask)
    _close("d_trans", d_trans, ref["d_trans"], 1e-5, 1e-4)
    _close("dx", dx[:, :d], ref["dx"], 1e-5, 1e-4)
    if gated:
        _close("d_alpha", d_alpha, ref["d_alpha"], 1e-4, 1e-4)
        assert d_alpha[3].item() == 0.0
    if use_norm:
        rows = 1 if shared else T
        _close("d_ln_w", d_lnw[:rows], ref["d_ln_w"], 1e-4, 1e-4)
        _close("d_ln_b", d_lnb[:rows], ref["d_ln_b"], 1e-4, 1e-4)
        if shared:
            assert bool((d_lnw[1:] == 3.0).all()), "shared norm wrote past row 0"
        else:
            assert bool((d_lnw[3] == 0).all() and (d_lnb[3] == 0).all()), "a type without rows gets zeros"


@pytest.mark.parametrize("m,n_cols,n", [(256, 256, 5000), (768, 256, 3000), (64, 37, 1000), (100, 400, 700), (128, 64, 300000), (96, 96, 0)])
def test_typed_weight_gradient_det_kernels(m, n_cols, n):
    """The shapes of test_typed_weight_gradient_kernels + 300 000 rows (147 chunks per group: the two-pass reduce) + no rows at all;
    group 1 has no rows.  Bounds of that test: 1e-4 * scale (weights), 1e-3 (column sums)."""
    lib = _lib.load()
    T = 3
    g = torch.Generator().manual_seed(m + n)
    A, B = torch.randn(n, m, generator=g), torch.randn(n, n_cols, generator=g)
    types = torch.randint(0, T + 1, (n,), generator=g)
    types[types == 1] = 2                                       # a group with zero rows
    order = torch.argsort(types, stable=True).to(torch.int32)
    off = torch.zeros(T + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.bincount(types, minlength=T + 1)[:T], 0)
    Ad, Bd, od, fd = A.to(DEV), B.to(DEV), order.to(DEV), off.to(DEV)
    if n == 0:
        Ad, Bd, od = torch.zeros(1, m, device=DEV), torch.zeros(1, n_cols, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ws, nb = _ws("hgt_typed_wgrad_det", T, n, m, n_cols)
    ws3, nb3 = _ws("hgt_typed_wgrad_bf16x3_det", T, n, m, n_cols)
    wsc, nbc = _ws("hgt_typed_colsum_det", T, n, m)
    print("wgrad det workspaces: fp32 %d, bf16x3 %d, colsum %d bytes" % (nb, nb3, nbc))
    runs = []
    for _ in range(2):
        out, out3 = torch.full((T, m, n_cols), 9.0, device=DEV), torch.full((T, m, n_cols), 9.0, device=DEV)
        cs, cs3 = torch.full((T, m), 9.0, device=DEV), torch.full((T, m), 9.0, device=DEV)
        assert lib.hgt_typed_wgrad_det(Ad.data_ptr(), m, Bd.data_ptr(), n_cols, od.data_ptr(), fd.data_ptr(), T, n, m, n_cols, out.data_ptr(),
                                       m * n_cols, ws.data_ptr(), nb, _st()) == 0
        assert lib.hgt_typed_colsum_det(Ad.data_ptr(), m, od.data_ptr(), fd.data_ptr(), T, n, m, cs.data_ptr(), m, wsc.data_ptr(), nbc, _st()) == 0
        assert lib.hgt_typed_wgrad_bf16x3_det(Ad.data_ptr(), m, Bd.data_ptr(), n_cols, od.data_ptr(), fd.data_ptr(), T, n, m, n_cols,
                                              out3.data_ptr(), m * n_cols, cs3.data_ptr(), m, ws3.data_ptr(), nb3, _st()) == 0
        torch.cuda.synchronize()
        runs.append((out, out3, cs, cs3))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    out, out3, cs, cs3 = runs[0]
    for t in range(T):
        idx = (types == t).nonzero().flatten()
        ref = A[idx].double().T @ B[idx].double()
        scale = max(1.0, ref.abs().max().item())
        for name, got in (("fp32", out), ("bf16x3", out3)):
            err = (got[t].cpu().double() - ref).abs().max().item()
            print("wgrad det %s group %d (%d rows): max err %.2e (bound %.2e)" % (name, t, idx.numel(), err, 1e-4 * scale))
            assert err < 1e-4 * scale
        assert (cs[t].cpu().double() - A[idx].double().sum(0)).abs().max().item() < 1e-3
        assert (cs3[t].cpu().double() - A[idx].double().sum(0)).abs().max().item() < 1e-3
    assert bool((out[1] == 0).all() and (out3[1] == 0).all() and (cs[1] == 0).all() and (cs3[1] == 0).all())


OUTER_DET_CASES = [
    # name, d, H, T, R, N, E, rte      (relation 1 has no edges wherever R > 1)
    ("valu16_r1_small", 64, 4, 3, 1, 3000, 24000, True),
    ("valu64_r33_large_plain", 256, 4, 3, 33, 66000, 500000, False),
    ("mfma_d256h8_small", 256, 8, 4, 8, 4000, 40000, True),
    ("mfma_d256h8_large_plain", 256, 8, 4, 33, 66000, 500000, False),
    ("mfma_d96h3_large_rte", 96, 3, 2, 33, 70000, 500000, True),           # padded heads
    ("w128_d768h8_r8_small_plain", 768, 8, 3, 8, 4000, 30000, False),
    ("w128_d768h8_r33_large_rte", 768, 8, 3, 33, 66000, 500000, True),
    ("w256_d768h4_r1_small_plain", 768, 4, 2, 1, 3000, 24000, False),
    ("tiny_one_slot", 64, 4, 2, 2, 40, 60, False),
]


@pytest.mark.parametrize("case", OUTER_DET_CASES, ids=[c[0] for c in OUTER_DET_CASES])
def test_relation_outer_det(case):
    name, d, H, T, R, N, E, rte = case
    lib = _lib.load()
    lay = BK._layout(d, H)
    Hl, dkp, dp = lay.heads, lay.dk_pad, lay.d_pad
    fn = "hgt_relation_outer_det" if dkp <= 64 else "hgt_relation_outer_wide_det"
    nt, ei, et, tm = BK._graph(N, E, T, R, seed=N + R + d, rte=rte, empty_rel=min(1, R - 1) if R > 1 else None)
    plan = GraphPlan(nt, ei, et, tm, T, R)
    g = _gen(d + H)
    w_id, a, b = _randn((E, Hl), g), _randn((N, dp), g), _randn((N, dp), g)
    rte_a = _randn((T * 240, dp), g) if rte else None
    w = BK._to_sorted(plan, w_id, T, R)
    ws, nb = _ws(fn, N, E, T, R, Hl, dkp)
    print("%s %s: workspace %d bytes" % (fn, name, nb))
    outs = []
    for _ in range(2):
        out = torch.full((R, Hl, dkp, dkp), 9.0, device=DEV)                # overwritten
        assert getattr(lib, fn)(plan.ptr, N, E, T, R, Hl, dkp, w.data_ptr(), a.data_ptr(), _p(rte_a), b.data_ptr(), out.data_ptr(),
                                ws.data_ptr(), nb, _st()) == 0
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    src, dst, rel, rrow = BP.plan_edges(nt, ei, et, tm, T, R)
    ref = BP.relation_outer(src, dst, rel, rrow, w_id, a, rte_a, b, R, Hl, dkp)
    if R > 1:
        assert bool((rel == 1).sum() == 0) and bool((outs[0][1] == 0).all()), "a relation without edges gets zeros"
    _close(fn, outs[0], ref, 2e-5, 1e-4)


@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "transposed"])
@pytest.mark.parametrize("case", [BK.SPMM_CASES[0], BK.SPMM_CASES[3], BK.SPMM_CASES[4]], ids=lambda c: c[0])
def test_edge_spmm_det(case, transposed):
    """hgt_edge_spmm with the deterministic hub mode: a target with > 1024 in-edges / a source with > 1024 out-edges (transposed)."""
    name, d, H, T, R, N, E, rte, nq = case
    lib = _lib.load()
    lay = BK._layout(d, H)
    Hl, dkp, dp = lay.heads, lay.dk_pad, lay.d_pad
    nt, ei, et, tm = BK._graph(N, E, T, R, seed=E + d, rte=rte, hubs=True)
    plan = GraphPlan(nt, ei, et, tm, T, R, reverse=transposed)
    src, dst, rel, rrow = BP.plan_edges(nt, ei, et, tm, T, R, reverse=transposed)
    assert torch.bincount(dst, minlength=N).max().item() > 1024, "no hub target in this plan"
    g = _gen(N + R)
    w_id, rows = _randn((E, Hl), g), _randn((N, dp), g)
    rte_rows = _randn((T * 240, dp), g) if rte else None
    f_p = (torch.randn(R, Hl, dkp, dkp, generator=g, device=DEV) / dkp ** 0.5)
    frag = BK._frags(f_p, R, Hl, dkp)
    w = BK._to_sorted(plan, w_id, T, R)
    ref = BP.edge_spmm(src, dst, rel, rrow, w_id, rows, rte_rows, f_p, N, R, Hl, dkp)
    ws, nb = _ws("hgt_edge_spmm_det", E, Hl, dkp, R)
    outs = []
    for _ in range(2):
        out = torch.full((N, 2 * dp), 5.0, device=DEV)
        assert lib.hgt_edge_spmm_det(plan.ptr, N, E, T, R, Hl, dkp, w.data_ptr(), rows.data_ptr(), _p(rte_rows), f_p.data_ptr(),
                                     frag.data_ptr(), out.data_ptr() + 4 * dp, 2 * dp, N, ws.data_ptr(), nb, _st()) == 0
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0][:, :dp] == 5.0).all())
    _close("spmm_det/%s" % name, outs[0][:, dp:], ref, 2e-5)


def test_small_workspace_is_refused_on_the_device_too():
    lib = _lib.load()
    T, n, m, n_cols = 3, 300000, 128, 64
    ws, nb = _ws("hgt_typed_wgrad_det", T, n, m, n_cols)
    assert nb > 0
    A, B = torch.zeros(n, m, device=DEV), torch.zeros(n, n_cols, device=DEV)
    rows = torch.arange(n, dtype=torch.int32, device=DEV)
    off = torch.tensor([0, n, n, n], dtype=torch.int32, device=DEV)
    out = torch.full((T, m, n_cols), 9.0, device=DEV)
    assert lib.hgt_typed_wgrad_det(A.data_ptr(), m, B.data_ptr(), n_cols, rows.data_ptr(), off.data_ptr(), T, n, m, n_cols, out.data_ptr(),
                                   m * n_cols, ws.data_ptr(), nb - 4, _st()) == -3
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()), "a refused call launched something"


# ------------------------------------------------------------------------------------------------------------------------------
# per layer
# ------------------------------------------------------------------------------------------------------------------------------
LAYER_CASES = [
    # name, class, T, R, H, d, N, E, use_norm, use_RTE, precision, graph kwargs, tweaks
    ("hgt_rte_norm_f16x3", HGTConv, 3, 4, 4, 64, 2000, 10000, True, True, "f16x3", {}, {}),
    ("hgt_plain_hubs_fp32", HGTConv, 3, 5, 2, 32, 3000, 30000, False, False, "fp32", dict(dst_skew=1.1), dict(hub=True, unclaimed=True)),
    ("hgt_d256h8_bf16x3", HGTConv, 4, 8, 8, 256, 4000, 40000, True, False, "bf16x3", {}, {}),
    ("hgt_d96h3_rte_bf16x3", HGTConv, 2, 3, 3, 96, 1200, 9000, True, True, "bf16x3", {}, dict(unknown=True)),
    ("hgt_d768h8_rte_f16x3", HGTConv, 2, 3, 8, 768, 1000, 7000, True, True, "f16x3", {}, {}),
    ("dense_rte_norm_bf16x3", DenseHGTConv, 3, 4, 4, 64, 2000, 10000, True, True, "bf16x3", {}, {}),
    ("dense_plain_fp32", DenseHGTConv, 2, 3, 4, 128, 1500, 9000, False, False, "fp32", dict(sorted_types=False), dict(unknown=True)),
    ("dense_d256h8_hubs_f16x3", DenseHGTConv, 4, 8, 8, 256, 3000, 30000, True, False, "f16x3", {}, dict(hub=True)),
]


def _slot_grads(layer, xd):
    """{name: gradient} of x and of every parameter (everything TENSOR_SLOTS packs comes from these parameters)."""
    g = {"x": xd.grad.clone()}
    for k, p in layer.named_parameters():
        if p.grad is not None:
            g[k] = p.grad.clone()
    return g


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_layer_gradients_repeat_bit_for_bit_and_match_the_oracle(case, monkeypatch):
    """Training mode, dropout 0.2 under a fixed seed: two steps give the same bits in every gradient; against the fp64 oracle with the
    masks the forward drew, at the tolerances of tests/test_backward_gpu.py."""
    name, cls, T, R, H, d, N, E, use_norm, use_RTE, precision, gk, tw = case
    dense = cls is DenseHGTConv
    p = 0.2
    assert len(TENSOR_SLOTS) == 20
    sd = O.make_state_dict(d, d, T, R, H, use_norm, use_RTE, seed=11, dense=dense)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=12, **gk)
    nt, et, ei = nt.clone(), et.clone(), ei.clone()
    if tw.get("unknown"):
        nt[::13] = T + 1
    if tw.get("unclaimed"):
        et[::7] = R
    if tw.get("hub"):
        ei[1, :4000] = 17                   # > 1024 in-edges ...
        ei[0, 4000:7000] = 23               # ... and > 1024 out-edges: a hub of the transposed plan
        assert torch.bincount(ei[1], minlength=N).max().item() > 1024 and torch.bincount(ei[0], minlength=N).max().item() > 1024
    assert spmm_takes_items(N, E, R, 4, 0)
    layer = cls(d, d, T, R, H, p, use_norm, use_RTE, precision=precision, deterministic=True)
    layer.load_state_dict(sd)
    layer = layer.to(DEV).train()
    drawn = []
    real_bernoulli = torch.bernoulli

    def recording_bernoulli(*a, **k):
        out = real_bernoulli(*a, **k)
        drawn.append(out.clone())
        return out

    monkeypatch.setattr(torch, "bernoulli", recording_bernoulli)
    gout = torch.randn(N, d, generator=torch.Generator().manual_seed(5))
    dev = [t.to(DEV) for t in (nt, ei, et)] + [tm.to(DEV) if use_RTE else None]
    runs, outs = [], []
    for _ in range(2):
        torch.manual_seed(1234)
        layer.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_(True)
        GraphPlan.clear_cache()
        out = layer(xd, *dev)
        out.backward(gout.to(DEV))
        torch.cuda.synchronize()
        runs.append(_slot_grads(layer, xd))
        outs.append(out.detach().clone())
    monkeypatch.undo()
    assert torch.equal(outs[0], outs[1])
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), "%s differs between two runs" % k
    n_masks = 2 if dense else 1
    assert len(drawn) == 2 * n_masks and torch.equal(drawn[0], drawn[n_masks])
    masks = [(m / (1.0 - p)).cpu() for m in drawn[:n_masks]]
    dm = (masks[0], masks[1] if dense else None)
    tme = tm if use_RTE else None
    fwd = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tme, use_norm=use_norm, use_RTE=use_RTE, dense=dense, drop_masks=dm)
    assert (outs[0].cpu().double() - fwd).abs().max().item() < 1e-4
    ref = O.backward_reference(sd, T, R, H, x, nt, ei, et, tme, gout, use_norm=use_norm, use_RTE=use_RTE, dense=dense, drop_masks=dm)
    worst = 0.0
    for k, got in runs[0].items():      # every figure first, then the assertions
        r64 = ref[k].to(torch.float64)
        print("det %s: %-28s max err %.2e of the largest entry" % (
            name, k, (got.cpu().double() - r64).abs().max().item() / max(r64.abs().max().item(), 1e-12)))
    for k, got in runs[0].items():
        worst = max(worst, _grads_close(k, got, ref[k]))
    assert set(runs[0]) >= {k for k, _ in layer.named_parameters() if k != "emb.emb.weight"} | {"x"}
    print("det layer %s: worst relative gradient error %.2e over %d tensors" % (name, worst, len(runs[0])))


@pytest.mark.parametrize("cls", [HGTConv, DenseHGTConv], ids=["hgt", "dense"])
def test_layer_above_the_item_threshold_with_hubs(cls):
    """N > 65 536: the gather passes take hgt_edge_spmm (sub-tile kernel + the hub path), the node update 32-row wavefronts' sizes,
    the outer products the large regime.  Two runs bit-equal; the oracle on a sample of targets (sampled_backward_check)."""
    dense = cls is DenseHGTConv
    T, R, H, d, N, E = 3, 4, 4, 64, 70000, 400000
    assert not spmm_takes_items(N, E, R, 3 * 64, 0)
    g = torch.Generator(device=DEV).manual_seed(77)
    nt = torch.randint(0, T, (N,), generator=g, device=DEV)
    x = torch.randn(N, d, generator=g, device=DEV)
    src = torch.randint(0, N, (E,), generator=g, device=DEV)
    dst = torch.randint(0, N, (E,), generator=g, device=DEV)
    dst[:1500] = 17
    src[2000:3600] = 23
    et = torch.randint(0, R, (E,), generator=g, device=DEV)
    tm = torch.randint(0, 240, (E,), generator=g, device=DEV)
    ei = torch.stack([src, dst], dim=1).t()
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=9, dense=dense)
    layer = cls(d, d, T, R, H, 0.2, True, True, precision="bf16x3", deterministic=True)
    layer.load_state_dict(sd)
    layer = layer.to(DEV).train()
    gout = torch.randn(N, d, generator=g, device=DEV)
    runs = []
    for _ in range(2):
        torch.manual_seed(99)
        layer.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        GraphPlan.clear_cache()
        layer(xd, nt, ei, et, tm).backward(gout)
        torch.cuda.synchronize()
        runs.append(_slot_grads(layer, xd))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), "%s differs between two runs" % k
    layer.eval()
    layer.zero_grad(set_to_none=True)
    BG.sampled_backward_check(layer, sd, (x, nt, ei, et, tm), (T, R, H, d), True, True, dense=dense,
                              extra_targets=torch.tensor([17, 23], device=DEV), label="deterministic, N = 70 000")


# ------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------
def _train_three_steps(deterministic, conv_name="hgt"):
    T, R, H, in_dim, d, N, E, n_cls = 3, 4, 4, 37, 64, 1200, 8000, 5
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, in_dim, T, R, seed=21)
    torch.manual_seed(1)
    gnn = GNN(in_dim, d, T, R, H, 2, dropout=0.2, conv_name=conv_name, prev_norm=True, last_norm=True, use_RTE=True).to(DEV).train()
    head = Classifier(d, n_cls).to(DEV).train()
    model = torch.nn.ModuleList([gnn, head])
    if deterministic:
        pyhgt_amd.set_deterministic(model, True)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    y = torch.randint(0, n_cls, (200,)).to(DEV)
    dev = [t.to(DEV) for t in (x, nt, tm, ei, et)]
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        rep = gnn(*dev)
        loss = torch.nn.functional.nll_loss(head(rep[:200]), y)      # seed rows as a slice
        loss.backward()
        opt.step()
        losses.append(loss.item())
    torch.cuda.synchronize()
    return [p.detach().clone() for p in model.parameters()], losses


@pytest.mark.parametrize("conv_name", ["hgt", "dense_hgt"])
def test_three_adamw_steps_repeat_bit_for_bit(conv_name):
    GraphPlan.clear_cache()
    p1, l1 = _train_three_steps(True, conv_name)
    GraphPlan.clear_cache()
    p2, l2 = _train_three_steps(True, conv_name)
    assert l1 == l2
    assert len(p1) == len(p2) and all(torch.equal(a, b) for a, b in zip(p1, p2))
    GraphPlan.clear_cache()
    _, l0 = _train_three_steps(False, conv_name)
    print("losses deterministic %s / default %s" % (l1, l0))
    assert all(abs(a - b) < 1e-4 for a, b in zip(l1, l0))            # the bound of test_gnn_training_step_matches_autograd_through_the_oracle


# ------------------------------------------------------------------------------------------------------------------------------
# guards
# ------------------------------------------------------------------------------------------------------------------------------
def test_unsupported_layout_still_raises_its_reason():
    T, R, H, d, N, E = 2, 2, 1, 512, 200, 1000
    ok, reason = training_supported(d, H)
    assert not ok
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=3)
    layer = HGTConv(d, d, T, R, H, 0.2, True, False, deterministic=True).to(DEV).train()
    with pytest.raises(NotImplementedError) as e:
        layer(x.to(DEV).requires_grad_(True), nt.to(DEV), ei.to(DEV), et.to(DEV), None)
    assert reason in str(e.value)


@pytest.mark.parametrize("cls", [HGTConv, DenseHGTConv], ids=["hgt", "dense"])
def test_false_is_the_attribute_never_set(cls, monkeypatch):
    """deterministic=False and a module without the attribute (a pickle of the reference class) take the same route and give the same
    bits.  The graph is small enough for every atomic of the default path to be the only addition to its address (one wavefront per
    node update, one chunk per group, one slice of the item list), so the default path itself repeats here; and no `_det` entry
    point is called in either state."""
    T, R, H, d, N, E = 2, 2, 2, 32, 2, 6
    lib = _lib.load()
    called = []
    for n in list(_lib.SIGNATURES):
        if n.endswith("_det"):
            real = getattr(lib, n)
            monkeypatch.setattr(lib, n, (lambda *a, _n=n, _r=real: (called.append(_n), _r(*a))[1]))
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(1))
    nt = torch.tensor([0, 1])
    ei = torch.tensor([[0, 1, 0, 1, 1, 0], [1, 0, 0, 1, 0, 1]])
    et = torch.tensor([0, 1, 1, 0, 0, 1])
    tm = torch.tensor([3, 7, 0, 100, 239, 5])
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=5, dense=cls is DenseHGTConv)
    results = []
    for state in ("false", "unset"):
        layer = cls(d, d, T, R, H, 0.2, True, True, deterministic=False)
        layer.load_state_dict(sd)
        if state == "unset":
            del layer.__dict__["deterministic"]
            assert "deterministic" not in layer.__dict__
        layer = layer.to(DEV).train()
        torch.manual_seed(4)
        xd = x.to(DEV).requires_grad_(True)
        GraphPlan.clear_cache()
        out = layer(xd, nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV))
        out.square().sum().backward()
        torch.cuda.synchronize()
        results.append((out.detach().clone(), _slot_grads(layer, xd)))
    assert called == []
    assert torch.equal(results[0][0], results[1][0])
    for k in results[0][1]:
        assert torch.equal(results[0][1][k], results[1][1][k]), k
    # and the switch does move the route
    layer = cls(d, d, T, R, H, 0.2, True, True, deterministic=True)
    layer.load_state_dict(sd)
    layer = layer.to(DEV).train()
    GraphPlan.clear_cache()
    layer(x.to(DEV).requires_grad_(True), nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV)).square().sum().backward()
    torch.cuda.synchronize()
    assert {"hgt_node_update_bwd_det", "hgt_relation_outer_det"} <= set(called)
    assert any(n.startswith("hgt_typed_wgrad") for n in called)
