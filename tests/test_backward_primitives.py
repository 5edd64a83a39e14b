"""CPU tests: the float64 restatements of the backward primitives (oracle/backward_primitives.py, what
tests/test_backward_kernels_gpu.py compares the kernels with) against reverse mode through the fp64 closed form
(oracle.hgt_oracle.forward_closed_form / backward_reference) on tiny graphs.  The gradients are chained together the way
pyhgt_amd/autograd.py chains the kernels, so these tests also pin the derivation the backward pass is built on."""
import math

import pytest
import torch

from oracle import backward_primitives as BP
from oracle import hgt_oracle as O
from pyhgt_amd.synth import synthetic_typed_graph

F64 = torch.float64


def _close(name, got, ref, tol=1e-9):
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got.to(F64) - ref.to(F64)).abs().max().item() / scale
    assert err < tol, "%s: %.3e of the largest entry" % (name, err)


def _typed(sd, fmt, x, nt, T, bias=True):
    """rows of type t: x W[t]^T + b[t]; rows of unknown type: 0 (conv.py:96-97,103 / 125)."""
    out = torch.zeros(x.size(0), sd[fmt % (0, "weight")].shape[0], dtype=F64)
    for t in range(T):
        r = (nt == t).nonzero(as_tuple=True)[0]
        out[r] = x[r] @ sd[fmt % (t, "weight")].to(F64).T + (sd[fmt % (t, "bias")].to(F64) if bias else 0.0)
    return out


def _typed_t(sd, fmt, dy, nt, T):
    """dy W[t] per row of type t (the input gradient of _typed)."""
    out = torch.zeros(dy.size(0), sd[fmt % (0, "weight")].shape[1], dtype=F64)
    for t in range(T):
        r = (nt == t).nonzero(as_tuple=True)[0]
        out[r] = dy[r] @ sd[fmt % (t, "weight")].to(F64)
    return out


def _case(use_rte, masked, seed):
    T, R, H, d, N, E = 3, 4, 2, 16, 70, 400
    sd = O.make_state_dict(d, d, T, R, H, True, use_rte, seed=seed)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=seed + 1, sorted_types=False)
    nt, et = nt.clone(), et.clone()
    nt[::11] = T + 1                      # unknown types
    et[::9] = R                           # unclaimed edges
    ei = ei.clone()
    ei[1, :60] = 5                        # a target with many in-edges
    g = torch.Generator().manual_seed(seed + 2)
    gout = torch.randn(N, d, generator=g, dtype=F64)
    m1 = (torch.bernoulli(torch.full((N, d), 0.7), generator=g) / 0.7).to(F64) if masked else None
    return T, R, H, d, N, E, sd, x.to(F64), nt, ei, et, (tm if use_rte else None), gout, m1


@pytest.mark.parametrize("use_rte,masked", [(True, False), (False, True), (True, True)])
def test_primitives_chain_to_the_oracle_gradients(use_rte, masked):
    """Every gradient of backward_reference rebuilt from the primitives: node_update_bwd + gelu_bwd (update), the logits-form
    d att, head_dot + edge_softmax_bwd (softmax), relation_outer (relation_msg / relation_att / relation_pri), edge_spmm on the
    plan and on the transposed plan (dQ / dK / dV -> bias gradients and dx)."""
    T, R, H, d, N, E, sd, x, nt, ei, et, tm, gout, m1 = _case(use_rte, masked, seed=40 + 2 * use_rte + masked)
    dk = d // H
    ref = O.backward_reference(sd, T, R, H, x, nt, ei, et, tm, gout, use_RTE=use_rte, drop_masks=(m1, None) if masked else None)
    out, att, agg = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, use_RTE=use_rte, return_att=True, return_agg=True,
                                          drop_masks=(m1, None) if masked else None)
    # ---- update (conv.py:119-133)
    g = O._gelu_erf(agg)
    trans = _typed(sd, "a_linears.%d.%s", g, nt, T)
    if masked:
        trans = trans * m1
    nub = BP.node_update_bwd(gout, trans, x, nt, T, skip=sd["skip"], ln_w=torch.stack([sd["norms.%d.weight" % t] for t in range(T)]),
                             drop_mask=m1)
    alpha = torch.sigmoid(sd["skip"].to(F64))
    _close("skip", nub["d_alpha"] * alpha * (1 - alpha), ref["skip"])
    for t in range(T):
        _close("norms.%d.weight" % t, nub["d_ln_w"][t], ref["norms.%d.weight" % t])
        _close("norms.%d.bias" % t, nub["d_ln_b"][t], ref["norms.%d.bias" % t])
        r = (nt == t).nonzero(as_tuple=True)[0]
        _close("a_linears.%d.weight" % t, nub["d_trans"][r].T @ g[r], ref["a_linears.%d.weight" % t])
        _close("a_linears.%d.bias" % t, nub["d_trans"][r].sum(0), ref["a_linears.%d.bias" % t])
    dagg = BP.gelu_bwd(_typed_t(sd, "a_linears.%d.%s", nub["d_trans"], nt, T), agg)
    # ---- projections and temporal tables (conv.py:91-92,96-97,103)
    Q, K, V = (_typed(sd, n + "_linears.%d.%s", x, nt, T) for n in ("q", "k", "v"))
    rte_k = rte_v = None
    if use_rte:
        rte = sd["emb.emb.weight"].to(F64) @ sd["emb.lin.weight"].to(F64).T + sd["emb.lin.bias"].to(F64)
        rte_k = torch.cat([rte @ sd["k_linears.%d.weight" % t].to(F64).T for t in range(T)])       # [T * 240, d]
        rte_v = torch.cat([rte @ sd["v_linears.%d.weight" % t].to(F64).T for t in range(T)])
    src, dst, rel, rrow = BP.plan_edges(nt, ei, et, tm, T, R)
    A, M, pri = sd["relation_att"].to(F64), sd["relation_msg"].to(F64), sd["relation_pri"].to(F64)
    # the aggregation itself is an edge_spmm with the attention as weights and F = M
    _close("agg = spmm(att, V, M)", BP.edge_spmm(src, dst, rel, rrow, att, V, rte_v, M, N, R, H, dk), agg)
    # ---- attention backward
    d_msg = BP.relation_outer(src, dst, rel, rrow, att, V, rte_v, dagg, R, H, dk)
    _close("relation_msg", d_msg, ref["relation_msg"])
    v_e = V[src] + (rte_v[rrow] if use_rte else 0.0)
    d_att = torch.zeros(E, H, dtype=F64)
    for r in range(R):                                  # hgt_edge_logits with (Q, K, att_t) := (dagg, V, M^T)
        s = (rel == r).nonzero(as_tuple=True)[0]
        d_att[s] = torch.einsum("ehk,hkc,ehc->eh", v_e[s].view(-1, H, dk), M[r], dagg[dst[s]].view(-1, H, dk))
    rho = BP.head_dot(dagg, agg, H, dk)
    ds = BP.edge_softmax_bwd(att, d_att, rho, dst)
    scale = (pri / math.sqrt(dk)).view(R, H, 1, 1)
    o_att = BP.relation_outer(src, dst, rel, rrow, ds, K, rte_k, Q, R, H, dk)
    _close("relation_att", o_att * scale, ref["relation_att"])
    _close("relation_pri", (o_att * A).sum(dim=(2, 3)) / math.sqrt(dk), ref["relation_pri"])
    # ---- dQ on the plan, dK / dV on the transposed plan
    dQ = BP.edge_spmm(src, dst, rel, rrow, ds, K, rte_k, A * scale, N, R, H, dk)
    ts, tt, trel, trrow = BP.plan_edges(nt, ei, et, None, T, R, reverse=True)
    dK = BP.edge_spmm(ts, tt, trel, trrow, ds, Q, None, (A * scale).transpose(2, 3), N, R, H, dk)
    dV = BP.edge_spmm(ts, tt, trel, trrow, att, dagg, None, M.transpose(2, 3), N, R, H, dk)
    for t in range(T):
        r = (nt == t).nonzero(as_tuple=True)[0]
        for n, dP in (("q", dQ), ("k", dK), ("v", dV)):
            _close("%s_linears.%d.bias" % (n, t), dP[r].sum(0), ref["%s_linears.%d.bias" % (n, t)])
    dx = nub["dx"] + sum(_typed_t(sd, n + "_linears.%d.%s", dP, nt, T) for n, dP in (("q", dQ), ("k", dK), ("v", dV)))
    _close("x", dx, ref["x"])


def test_node_update_bwd_restates_the_dense_update():
    """DenseHGTConv (conv.py:261-274): the shared out_norm through node_update_bwd(skip=None, shared_norm=True, mask m2) and the
    typed norms through node_update_bwd(skip=None, mask m1), chained through mid_linear / out_linear, give the oracle's gradients."""
    T, R, H, d, N, E = 3, 4, 2, 16, 60, 300
    sd = O.make_state_dict(d, d, T, R, H, True, False, seed=5, dense=True)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=6, sorted_types=False)
    nt = nt.clone()
    nt[::7] = -1
    x = x.to(F64)
    g = torch.Generator().manual_seed(7)
    gout = torch.randn(N, d, generator=g, dtype=F64)
    m1, m2 = ((torch.bernoulli(torch.full((N, d), 0.75), generator=g) / 0.75).to(F64) for _ in range(2))
    ref = O.backward_reference(sd, T, R, H, x, nt, ei, et, None, gout, use_RTE=False, dense=True, drop_masks=(m1, m2))
    _, agg = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, None, use_RTE=False, dense=True, return_agg=True, drop_masks=(m1, m2))
    Wm, bm, Wo, bo = (sd[k].to(F64) for k in ("mid_linear.weight", "mid_linear.bias", "out_linear.weight", "out_linear.bias"))
    trans = _typed(sd, "a_linears.%d.%s", agg, nt, T) * m1
    lnw = torch.stack([sd["norms.%d.weight" % t] for t in range(T)]).to(F64)
    lnb = torch.stack([sd["norms.%d.bias" % t] for t in range(T)]).to(F64)
    y = trans + x
    mu, var = y.mean(1, keepdim=True), y.var(1, unbiased=False, keepdim=True)
    tc = nt.clamp(0, T - 1)
    y1 = (y - mu) / torch.sqrt(var + 1e-5) * lnw[tc] + lnb[tc]
    mid = y1 @ Wm.T + bm
    trans2 = (O._gelu_erf(mid) @ Wo.T + bo) * m2
    b2 = BP.node_update_bwd(gout, trans2, y1, nt, T, ln_w=sd["out_norm.weight"].view(1, d), shared_norm=True, drop_mask=m2)
    ok = (nt >= 0) & (nt < T)
    _close("out_norm.weight", b2["d_ln_w"][0], ref["out_norm.weight"])
    _close("out_norm.bias", b2["d_ln_b"][0], ref["out_norm.bias"])
    _close("out_linear.bias", b2["d_trans"][ok].sum(0), ref["out_linear.bias"])
    d_mid = BP.gelu_bwd(b2["d_trans"] @ Wo, mid)
    _close("mid_linear.bias", d_mid[ok].sum(0), ref["mid_linear.bias"])
    d_y1 = b2["dx"] + (d_mid @ Wm) * ok.unsqueeze(1)
    b1 = BP.node_update_bwd(d_y1, trans, x, nt, T, ln_w=lnw, drop_mask=m1)
    for t in range(T):
        _close("norms.%d.weight" % t, b1["d_ln_w"][t], ref["norms.%d.weight" % t])
        _close("norms.%d.bias" % t, b1["d_ln_b"][t], ref["norms.%d.bias" % t])
        r = (nt == t).nonzero(as_tuple=True)[0]
        _close("a_linears.%d.bias" % t, b1["d_trans"][r].sum(0), ref["a_linears.%d.bias" % t])


def test_drop_masks_none_is_the_eval_oracle_bit_for_bit():
    T, R, H, d, N, E, sd, x, nt, ei, et, tm, gout, _ = _case(True, False, seed=3)
    a = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm)
    b = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, drop_masks=None)
    assert torch.equal(a, b)
    ones = torch.ones(N, d, dtype=F64)
    assert torch.equal(O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, drop_masks=(ones, None)), a)
    zeros = torch.zeros(N, d, dtype=F64)
    # p = 1: the a_linear output is dropped entirely -> out = LN(x (1 - alpha)) on the rows of known type
    z = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, drop_masks=(zeros, None))
    alpha = torch.sigmoid(sd["skip"].to(F64))
    for t in range(T):
        r = (nt == t).nonzero(as_tuple=True)[0]
        y = x[r] * (1 - alpha[t])
        exp = O._layer_norm(y, sd["norms.%d.weight" % t].to(F64), sd["norms.%d.bias" % t].to(F64))
        assert (z[r] - exp).abs().max().item() < 1e-12
