"""Plain float64 restatements of the backward primitives of include/hgt_hip.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Each function states the definition of one C-ABI primitive of the backward pass (include/hgt_hip.h, the block above
hgt_edge_spmm) in torch ops, without any of the kernels' tiling, so that tests/test_backward_kernels_gpu.py can call the
primitive through the C ABI and compare.  tests/test_backward_primitives.py checks these restatements against reverse
mode through oracle.hgt_oracle.forward_closed_form / _update on tiny graphs.

The functions run on whatever device their inputs live on (torch's own kernels in float64: on the GPU for the large
shapes of the kernel tests, on the CPU in the CPU tests).  Edge-level primitives take the edges in ORIGINAL edge order,
classified the way hgt_plan_build does (plan_edges): an edge is claimed by relation r when its relation id is r and
both endpoint types are in [0, T); every other edge belongs to the "unclaimed" bucket R, which carries no message.
"""
import math

import torch

RTE_LEN = 240   # HGT_RTE_LEN: rows of a temporal table per source type


def plan_edges(node_type, edge_index, edge_type, edge_time, num_types, num_relations, reverse=False):
    """(src, dst, rel, rte_row) per original edge, as a plan of the graph (reverse=True: of the transposed graph) sees it:
    rel = R for unclaimed edges; rte_row = type(src) * 240 + edge_time (time 0 without edge_time; an unknown source type
    counts as type 0, like the plan build's clamp)."""
    T, R = int(num_types), int(num_relations)
    src, dst = edge_index[0].long(), edge_index[1].long()
    if reverse:
        src, dst = dst, src
    ts, td = node_type[src].long(), node_type[dst].long()
    et = edge_type.long()
    claimed = (ts >= 0) & (ts < T) & (td >= 0) & (td < T) & (et >= 0) & (et < R)
    rel = torch.where(claimed, et, torch.full_like(et, R))
    tm = edge_time.long() if edge_time is not None else torch.zeros_like(et)
    rte_row = torch.where((ts >= 0) & (ts < T), ts, torch.zeros_like(ts)) * RTE_LEN + tm
    return src, dst, rel, rte_row


def node_update_bwd(grad_out, trans, x, node_type, num_types, skip=None, ln_w=None, use_norm=True, shared_norm=False,
                    drop_mask=None):
    """hgt_node_update_bwd / hgt_node_update_bwd_ex.  Forward per row i of type t in [0, T):
        y = o a + x (1 - a), a = sigmoid(skip[t])      (skip None: y = o + x, the plain residual)
        out = LN(y) * w + b                            (w = ln_w[t], or ln_w[0] with shared_norm; no LN without use_norm)
    with o = trans[i] = the a_linear output AFTER the dropout mask (o = mask * u).  Returns float64
        d_trans = dL/du = mask * dL/do,  dx = dL/dx (skip path),  d_alpha[t] = dL/da = sum dy (o - x),
        d_ln_w, d_ln_b [T or 1][d]
    for L = <out, grad_out>, by reverse mode through that formula.  Rows of unknown type: d_trans = dx = 0."""
    f64 = torch.float64
    dev = grad_out.device
    N, d = trans.shape
    T = int(num_types)
    nt = node_type.long()
    o = trans.to(f64).detach().requires_grad_(True)
    xx = x[:, :d].to(f64).detach().requires_grad_(True)
    gate = skip is not None
    alpha = (torch.sigmoid(skip.to(f64)) if gate else torch.ones(T, dtype=f64, device=dev)).detach().requires_grad_(True)
    n_ln = 1 if shared_norm else T
    w = ln_w.to(f64)[:n_ln].detach().requires_grad_(True) if use_norm else None
    b = torch.zeros(n_ln, d, dtype=f64, device=dev, requires_grad=True) if use_norm else None
    ok = (nt >= 0) & (nt < T)
    tc = torch.where(ok, nt, torch.zeros_like(nt))
    a = alpha[tc].unsqueeze(1)
    y = o * a + xx * ((1.0 - a) if gate else 1.0)
    if use_norm:
        mu = y.mean(dim=1, keepdim=True)
        var = ((y - mu) ** 2).mean(dim=1, keepdim=True)
        li = torch.zeros_like(tc) if shared_norm else tc
        y = (y - mu) / torch.sqrt(var + 1e-5) * w[li] + b[li]
    loss = (y * grad_out.to(f64) * ok.unsqueeze(1).to(f64)).sum()
    leaves = [o, xx, alpha] + ([w, b] if use_norm else [])
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    d_trans = grads[0] * (drop_mask.to(f64) if drop_mask is not None else 1.0)
    res = {"d_trans": d_trans * ok.unsqueeze(1), "dx": grads[1] * ok.unsqueeze(1),
           "d_alpha": grads[2] if grads[2] is not None else torch.zeros(T, dtype=f64, device=dev)}
    if use_norm:
        res["d_ln_w"], res["d_ln_b"] = grads[3], grads[4]
    return res


def gelu_bwd(dg, agg):
    """hgt_gelu_bwd: dg * gelu'(agg), gelu = exact erf form (conv.py:119)."""
    v = agg.to(torch.float64)
    cdf = 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    return dg.to(torch.float64) * (cdf + v * pdf)


def head_dot(a, b, n_heads, dk_pad):
    """hgt_head_dot: rho[n][h] = <a[n][h*dk_pad : (h+1)*dk_pad], b[n][same columns]>."""
    n = a.shape[0]
    return (a.to(torch.float64).view(n, n_heads, dk_pad) * b.to(torch.float64).view(n, n_heads, dk_pad)).sum(-1)


def edge_softmax_bwd(att, d_att, rho, dst):
    """hgt_edge_softmax_bwd in edge-id order: d s_e = att_e (d att_e - rho[dst_e])."""
    return att.to(torch.float64) * (d_att.to(torch.float64) - rho.to(torch.float64)[dst])


def _source_rows(rows, rte_rows, src, rte_row, sel):
    a = rows.to(torch.float64)[src[sel]]
    if rte_rows is not None:
        a = a + rte_rows.to(torch.float64)[rte_row[sel]]
    return a


def relation_outer(src, dst, rel, rte_row, w, a_src, rte_a, b_dst, num_relations, n_heads, dk_pad):
    """hgt_relation_outer (without the += of the kernel):
        out[r][h][k][c] = sum_{e of relation r} w[e][h] (a_src[src_e] + rte_a[rte_row_e])[h][k] b_dst[dst_e][h][c]
    for r in [0, R) (the unclaimed bucket contributes nothing); w in original edge order [E][H]."""
    R, H, dkp = int(num_relations), int(n_heads), int(dk_pad)
    out = torch.zeros(R, H, dkp, dkp, dtype=torch.float64, device=w.device)
    for r in range(R):
        sel = (rel == r).nonzero(as_tuple=True)[0]
        if sel.numel() == 0:
            continue
        a = _source_rows(a_src, rte_a, src, rte_row, sel)[:, :H * dkp].view(-1, H, dkp) * w.to(torch.float64)[sel].unsqueeze(-1)
        b = b_dst.to(torch.float64)[dst[sel]][:, :H * dkp].view(-1, H, dkp)
        out[r] = torch.einsum("ehk,ehc->hkc", a, b)
    return out


def edge_spmm(src, dst, rel, rte_row, w, rows, rte_rows, f, n_out_rows, num_relations, n_heads, dk_pad):
    """hgt_edge_spmm / hgt_edge_spmm_items (out overwritten, rows [0, n_out_rows)):
        out[i][h][c] = sum_r sum_{e in (i, r)} w[e][h] sum_k (rows[src_e] + rte_rows[rte_row_e])[h][k] f[r][h][k][c]
    for r in [0, R); w in original edge order [E][H], f in the hgt_relation_pack layout [R][H][dk_pad][dk_pad]."""
    R, H, dkp = int(num_relations), int(n_heads), int(dk_pad)
    out = torch.zeros(int(n_out_rows), H, dkp, dtype=torch.float64, device=w.device)
    for r in range(R):
        sel = (rel == r).nonzero(as_tuple=True)[0]
        if sel.numel() == 0:
            continue
        a = _source_rows(rows, rte_rows, src, rte_row, sel)[:, :H * dkp].view(-1, H, dkp) * w.to(torch.float64)[sel].unsqueeze(-1)
        out.index_add_(0, dst[sel], torch.einsum("ehk,hkc->ehc", a, f.to(torch.float64)[r]))
    return out.view(int(n_out_rows), H * dkp)
