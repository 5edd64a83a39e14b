"""Whole task steps in plain torch on the CPU -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (see oracle/hgt_oracle.py).

A task step is what one iteration of the reference's training scripts computes between the sampled batch and `loss.backward()`:

    node_rep = GNN(batch)                               pyHGT/model.py:66-80 (eval mode: dropout is the identity)
    author   res  = Matcher(node_rep[author_key], node_rep[paper_key], pair=True)        model.py:16-46
             loss = mask_softmax(res, key_size)                                          OAG/train_author_disambiguation.py:90-96
    field    res  = Classifier(node_rep[x_ids]);  loss = KLDivLoss('batchmean')(res, ylabel)       OAG/train_paper_field.py
    venue    res  = Classifier(node_rep[x_ids]);  loss = NLLLoss()(res, ylabel)                    OAG/train_paper_venue.py

Everything is a differentiable torch op, float64 unless `dtype=` says otherwise (float32 is the yardstick of the tests: what a correct
single-precision implementation of the same formulas gives).  Parameters travel as one dict `P` keyed by state_dict name: the GNN's own
names, the Classifier's under `head.` and the Matcher's under `matcher.`.  A batch is a dict of CPU tensors:

    x [N, in_dim], node_type [N], edge_time [E], edge_index [2, E], edge_type [E]        the five tensors GNN.forward takes
    author:  paper_key [L], author_key [L] (rows of node_rep), sizes (the lengths of the consecutive segments of the L pairs)
    field:   rows [n], ylabel [n, C] (rows that sum to 1)
    venue:   rows [n], y [n] (class indices)
"""
import math

import numpy as np
import torch

from . import hgt_oracle as O

KINDS = ("author", "field", "venue")


def params_of(gnn, head, prefix, dtype=torch.float64):
    """leaf copies of the parameters of a GNN and of its head, by state_dict name (`prefix` = "head." or "matcher.")"""
    named = list(gnn.named_parameters()) + [(prefix + k, v) for k, v in head.named_parameters()]
    return {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in named}


def gnn_rep(P, num_types, num_relations, n_heads, n_layers, x, node_type, edge_time, edge_index, edge_type, dtype=torch.float64,
            prev_norm=True, last_norm=True, use_RTE=True):
    """GNN.forward (model.py:66-80) in eval mode, differentiable in P: the adapter as an index_add of tanh(x W_t^T + b_t) per type,
    then forward_closed_form per layer.  Same argument order as the module: edge_time comes third."""
    n_hid = P["adapt_ws.0.weight"].shape[0]
    x = x.to(dtype)
    h = torch.zeros(x.size(0), n_hid, dtype=dtype)
    for t in range(num_types):
        idx = (node_type == t).nonzero().flatten()
        h = h.index_add(0, idx, torch.tanh(x[idx] @ P["adapt_ws.%d.weight" % t].to(dtype).T + P["adapt_ws.%d.bias" % t].to(dtype)))
    for li in range(n_layers):
        pre = "gcs.%d.base_conv." % li
        sd = {k[len(pre):]: v for k, v in P.items() if k.startswith(pre)}
        h = O.forward_closed_form(sd, num_types, num_relations, n_heads, h, node_type, edge_index, edge_type, edge_time if use_RTE else None,
                                  use_norm=last_norm if li == n_layers - 1 else prev_norm, use_RTE=use_RTE, dtype=dtype)
    return h


# ---------------------------------------------------------------------------------------------------------------- heads (model.py:3-49)
def matcher_projections(P, rep, author_key, paper_key, prefix="matcher."):
    """(left_linear(rep[author_key]), right_linear(rep[paper_key])): tx and ty of Matcher.forward(rep[author_key], rep[paper_key])"""
    tx = rep[author_key] @ P[prefix + "left_linear.weight"].to(rep.dtype).T + P[prefix + "left_linear.bias"].to(rep.dtype)
    ty = rep[paper_key] @ P[prefix + "right_linear.weight"].to(rep.dtype).T + P[prefix + "right_linear.bias"].to(rep.dtype)
    return tx, ty


def matcher_pair(P, rep, author_key, paper_key, prefix="matcher.", projections=None):
    """Matcher.forward(rep[author_key], rep[paper_key], pair=True): the authors go through left_linear, the papers through right_linear"""
    tx, ty = matcher_projections(P, rep, author_key, paper_key, prefix) if projections is None else projections
    return (tx * ty).sum(dim=-1) / math.sqrt(P[prefix + "left_linear.weight"].shape[0])


def classifier(P, rep_rows, prefix="head."):
    """Classifier.forward: log_softmax(linear(x))"""
    return torch.log_softmax(rep_rows @ P[prefix + "linear.weight"].to(rep_rows.dtype).T + P[prefix + "linear.bias"].to(rep_rows.dtype), dim=-1)


# ---------------------------------------------------------------------------------------------------------------- losses
def mask_softmax_terms(pred, sizes):
    """the summands of mask_softmax (train_author_disambiguation.py:90-96), one per segment: -log_softmax(seg)[0] / ln(len)"""
    out, beg = [], 0
    for l in np.asarray(sizes).tolist():
        out.append(-torch.log_softmax(pred[beg:beg + l], dim=-1)[0] / math.log(l))
        beg += l
    return torch.stack(out)


def mask_softmax(pred, sizes):
    return mask_softmax_terms(pred, sizes).sum()


def kl_terms(logp, ylabel):
    """per row sum_c y (log y - logp), 0 where y = 0: the rows of nn.KLDivLoss(reduction='none')"""
    return torch.nn.functional.kl_div(logp, ylabel.to(logp.dtype), reduction="none").sum(dim=1)


def nll_terms(logp, y):
    return torch.nn.functional.nll_loss(logp, y, reduction="none")


def head_step(kind, P, rep, batch, projections=None):
    """head and loss of one step on a given node_rep -> (scores, per-row loss terms, loss); the loss is what the scripts' own calls
    give: mask_softmax, nn.KLDivLoss(reduction='batchmean'), nn.NLLLoss()"""
    if kind == "author":
        scores = matcher_pair(P, rep, batch["author_key"], batch["paper_key"], projections=projections)
        terms = mask_softmax_terms(scores, batch["sizes"])
        return scores, terms, terms.sum()
    scores = classifier(P, rep[batch["rows"]])
    if kind == "field":
        return scores, kl_terms(scores, batch["ylabel"]), torch.nn.KLDivLoss(reduction="batchmean")(scores, batch["ylabel"].to(scores.dtype))
    if kind == "venue":
        return scores, nll_terms(scores, batch["y"]), torch.nn.NLLLoss()(scores, batch["y"])
    raise ValueError("kind is one of %r" % (KINDS,))


def task_step(kind, P, batch, num_types, num_relations, n_heads, n_layers, dtype=torch.float64, **gnn_kw):
    """One whole step.  P: parameters by name (any float dtype; they are cast to `dtype` and made leaves here).
    -> {"rep", "scores", "terms", "loss", "grad_rep", "grads": {name: d loss / d parameter}}, all detached, in `dtype`; a parameter the
    loss does not depend on has a gradient of zeros.  The author step adds "grad_left" = d loss / d left_linear(rep[author_key]) [L, n_hid],
    the rows whose column sum is the gradient of the Matcher's left bias."""
    P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in P.items()}
    rep = gnn_rep(P, num_types, num_relations, n_heads, n_layers, batch["x"], batch["node_type"], batch["edge_time"], batch["edge_index"],
                  batch["edge_type"], dtype=dtype, **gnn_kw)
    proj = matcher_projections(P, rep, batch["author_key"], batch["paper_key"]) if kind == "author" else None
    scores, terms, loss = head_step(kind, P, rep, batch, projections=proj)
    names = list(P)
    wrt = [rep] + [P[k] for k in names] + ([proj[0]] if proj else [])
    grads = torch.autograd.grad(loss, wrt, allow_unused=True)
    zero = lambda g, like: torch.zeros_like(like) if g is None else g
    out = {"rep": rep.detach(), "scores": scores.detach(), "terms": terms.detach(), "loss": loss.detach(),
           "grad_rep": zero(grads[0], rep).detach(), "grads": {k: zero(g, P[k]).detach() for k, g in zip(names, grads[1:])}}
    if proj:
        out["grad_left"] = grads[-1].detach()
    return out
