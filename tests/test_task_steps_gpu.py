"""Whole task steps on the GPU against oracle/task_steps.py in float64: a batch drawn by the device sampler with its label edges masked,
GNN in training mode (dropout 0) -> Matcher(pair=True) -> pair_rank_loss (author disambiguation), -> Classifier -> KLDivLoss on
LabelSpace.distribution rows (paper-field) or nll_loss on LabelSpace.index (paper-venue), then loss.backward().  Checked per step:

  node_rep      against the float64 GNN on the host copy of the batch, max abs <= 1e-4 (the project's layer bound);
  heads, loss   on the device's own node_rep: scores and per-row loss terms against the float64 heads on that node_rep, gated by 4 x the
                error of the same heads in torch float32 on the CPU (the convention of tests/test_task_metrics_gpu.py); the inference
                path (eval, no_grad: hgt_row_dot / hgt_log_softmax_rows) the same way on its own node_rep;
  keys, labels  candidate_pairs against the script's loop in numpy; the label rows against np_label_* on a host twin of the graph;
  gradients     node_rep.grad and every parameter gradient under the gradient rules of tests/task_step_cases.py;
  metrics       rank_metrics against np_rank_metrics on the host copy of the same scores;
  determinism   with deterministic=True two steps from fresh modules agree bit for bit (author step).

The cancelling tensors of the author step (tests/task_step_cases.py: CANCELLING, with the algebra) are `matcher.left_linear.bias` and
`gcs.1.base_conv.norms.1.bias`, the LayerNorm bias of the author type in the last layer: both are column sums over rows whose
per-segment contributions add up to zero, because the paper is fixed within a segment and softmax minus one-hot sums to zero.  The
paper steps have none.  tests/test_task_steps.py pins the classes on the CPU and shows that float32 torch meets every rule."""
import time

import numpy as np
import pytest
import torch

import task_step_cases as TC
from oracle import hgt_oracle as O
from oracle import task_steps as TS
from pyhgt_amd import (GNN, Classifier, Matcher, Segments, np_label_distribution, np_label_index, np_rank_metrics, pair_rank_loss,
                       rank_metrics, sample_subgraph_device)
from test_backward_gpu import _grads_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REP_TOL, NDCG_TOL = 1e-4, 1e-12
PRECISIONS = ["bf16x3", "f16x3"]


@pytest.fixture(scope="module")
def author_world():
    ex, dgraph, first, year = TC.author_graph(DEV)
    return ex, dgraph, first, year


@pytest.fixture(scope="module")
def paper_world():
    ex, dgraph, n_nodes = TC.paper_graph(DEV)
    _, host, _ = TC.paper_graph(None)
    return ex, dgraph, n_nodes, host


def _modules(kind, dgraph, precision, n_out=None, deterministic=False):
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    gnn = GNN(TC.IN_DIM, TC.N_HID, T, R, TC.N_HEADS, TC.N_LAYERS, dropout=0, prev_norm=True, last_norm=True, use_RTE=True,
              deterministic=deterministic)
    gnn.load_state_dict(O.make_gnn_state_dict(TC.IN_DIM, TC.N_HID, T, R, TC.N_HEADS, TC.N_LAYERS, True, True, True, seed=TC.WEIGHT_SEED))
    for gc in gnn.gcs:
        gc.base_conv.precision = precision
    torch.manual_seed(TC.HEAD_SEED)
    head = Matcher(TC.N_HID, deterministic=deterministic) if kind == "author" else Classifier(TC.N_HID, n_out, deterministic=deterministic)
    return gnn.to(DEV).train(), head.to(DEV).train(), T, R


def _isolation(kind, P, rep_dev, batch, scores_dev, terms_dev, tag):
    """heads and loss on the device's own node_rep: float64 on the host as the truth, torch float32 on the host as the yardstick"""
    rep = rep_dev.detach().cpu()
    with torch.no_grad():
        s64, t64, _ = TS.head_step(kind, P, rep.double(), batch)
        s32, t32, _ = TS.head_step(kind, {k: v.detach().float() for k, v in P.items()}, rep, batch)
    out = []
    for what, dev, f64, f32 in (("scores", scores_dev, s64, s32), ("loss terms", terms_dev, t64, t32)):
        if dev is None:
            continue
        assert f32.dtype == torch.float32 and dev.shape == f64.shape
        err, yard = (dev.detach().cpu().double() - f64).abs().max().item(), (f32.double() - f64).abs().max().item()
        print("%s: %s on the device's node_rep: max err %.3e, torch float32 %.3e" % (tag, what, err, yard))
        assert err <= 4 * yard, "%s: %s miss 4 x the float32 yardstick: %.3e > 4 * %.3e" % (tag, what, err, yard)
        out.append((err, yard))
    return out


def _gradients(kind, gnn, head, node_rep, P, batch, T, R, tag):
    step = TS.task_step(kind, P, batch, T, R, TC.N_HEADS, TC.N_LAYERS)
    err_rep = (node_rep.detach().cpu().double() - step["rep"]).abs().max().item()
    print("%s: node_rep max err %.3e against float64" % (tag, err_rep))
    assert err_rep <= REP_TOL
    got = {k: v.grad for k, v in list(gnn.named_parameters()) + [(TC.PREFIX[kind] + k, v) for k, v in head.named_parameters()]}
    TC.check_gradient_rules(kind, got, step, P, batch["node_type"], tag)
    unread = ~step["grad_rep"].any(dim=1)                               # rows the loss does not read: exactly zero on the device too
    assert unread.any() and not node_rep.grad.cpu()[unread].any()
    print("%s: d loss / d node_rep: %.2e of the largest entry" % (tag, _grads_close("node_rep", node_rep.grad, step["grad_rep"], rtol=TC.GRAD_RTOL)))
    return step


# ---------------------------------------------------------------------------------------------------------------- a. the author step
def _author_step(world, precision, deterministic, check):
    ex, dgraph, first, year = world
    gnn, matcher, T, R = _modules("author", dgraph, precision, deterministic=deterministic)
    g, batch, name_label, (paper_key, author_key, sizes) = TC.host_author_batch(sample_subgraph_device, ex, dgraph, first, year)
    seg = Segments(sizes, DEV)
    node_rep = gnn(g[0], g[1], g[2], g[3], g[4])
    node_rep.retain_grad()
    res = matcher(node_rep[author_key], node_rep[paper_key], pair=True)
    loss = pair_rank_loss(res, seg)
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach(), "rep_grad": node_rep.grad, "grads": {k: v.grad for k, v in list(gnn.named_parameters()) + list(matcher.named_parameters())}}
    if not check:
        return out
    tag = "author step / %s%s" % (precision, " / deterministic" if deterministic else "")
    assert sizes.tolist() == TC.AUTHOR_SIZES and g.n_seed["author"] == TC.N_AUTHOR_SEEDS
    print("%s: %d nodes, %d edges, %d pairs" % (tag, g[1].numel(), g[4].numel(), seg.total))
    # 3. the keys are the script's loop on the host copy of the seeds' rows
    pk, ak, ks = TC.np_author_keys(g.seed_rows("paper").cpu().numpy(), g.seed_rows("author").cpu().numpy(), name_label)
    assert np.array_equal(paper_key.cpu().numpy(), pk) and np.array_equal(author_key.cpu().numpy(), ak) and np.array_equal(sizes, ks)
    assert np.unique(ak).size < ak.size and (g[1][author_key] == dgraph.types.index("author")).all() and (g[1][paper_key] == 0).all()
    # 2. heads and loss in isolation, training path and inference path
    P = TS.params_of(gnn, matcher, "matcher.")
    terms = pair_rank_loss(res.detach(), seg, reduce=False)
    assert res.dtype == torch.float32 and terms.shape == (len(TC.AUTHOR_SIZES),)
    _isolation("author", P, node_rep, batch, res, terms, tag)
    gnn.eval(), matcher.eval()
    with torch.no_grad():
        rep_inf = gnn(g[0], g[1], g[2], g[3], g[4])
        res_inf = matcher(rep_inf[author_key], rep_inf[paper_key], pair=True)
        assert not res_inf.requires_grad
        _isolation("author", P, rep_inf, batch, res_inf, pair_rank_loss(res_inf, seg, reduce=False), tag + " / inference path")
    gnn.train(), matcher.train()
    # 1. + 4. node_rep and the gradients of the whole chain
    step = _gradients("author", gnn, matcher, node_rep, P, batch, T, R, tag)
    print("%s: loss %.6f, float64 %.6f" % (tag, loss.item(), step["loss"].item()))
    # 5. metrics on the device against the rule on the host copy of the same scores
    ndcg, rr = rank_metrics(res.detach(), sizes=seg)
    want_ndcg, want_rr = np_rank_metrics(res.detach().cpu().numpy(), sizes=sizes)
    assert np.array_equal(rr.cpu().numpy(), want_rr) and np.abs(ndcg.cpu().numpy() - want_ndcg).max() <= NDCG_TOL
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
def test_author_step_against_float64(author_world, precision):
    t0 = time.perf_counter()
    _author_step(author_world, precision, False, True)
    print("author step / %s: %.2f s" % (precision, time.perf_counter() - t0))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_deterministic_author_step_against_float64_and_bit_for_bit(author_world, precision):
    """deterministic=True on GNN and Matcher: the rules hold on this route too, and two steps from fresh modules with equal weights give
    the same bits in the loss, in d loss / d node_rep and in every parameter gradient, although every paper row is gathered once per
    candidate and authors recur across the lists"""
    t0 = time.perf_counter()
    a = _author_step(author_world, precision, True, True)
    b = _author_step(author_world, precision, True, False)
    assert torch.equal(a["loss"], b["loss"]), (a["loss"].item(), b["loss"].item())
    assert torch.equal(a["rep_grad"], b["rep_grad"])
    differ = [k for k in a["grads"] if (a["grads"][k] is None) != (b["grads"][k] is None)
              or (a["grads"][k] is not None and not torch.equal(a["grads"][k], b["grads"][k]))]
    assert not differ, differ
    print("deterministic author step / %s: %d gradients bit-equal, %.2f s" % (precision, len(a["grads"]), time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------------------------- b., c. the paper steps
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["field", "venue"])
def test_paper_step_against_float64(paper_world, kind, precision):
    t0 = time.perf_counter()
    ex, dgraph, n_nodes, host = paper_world
    tag = "paper-%s step / %s" % (kind, precision)
    g, batch, space, labels = TC.host_paper_batch(sample_subgraph_device, kind, ex, dgraph, n_nodes)
    gnn, head, T, R = _modules(kind, dgraph, precision, n_out=space.n_cols)
    x_ids = g.seed_rows("paper")
    ids = g.indxs["paper"][:TC.N_PAPER_SEEDS].cpu().numpy()
    print("%s: %d nodes, %d edges, %d seeds, %d classes" % (tag, g[1].numel(), g[4].numel(), x_ids.numel(), space.n_cols))
    # the labels against the rule on the host twin of the graph
    if kind == "field":
        want = np_label_distribution(host, space.triple, space.col_of, space.n_cols, ids, *ex.TRAIN_YEARS)
        assert space.n_cols == TC.N_FIELDS and np.array_equal(labels.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert (labels.double().sum(dim=1) - 1).abs().max().item() <= TC.N_FIELDS * 2.0 ** -24 and (labels > 0).sum(dim=1).max().item() > 1
    else:
        assert np.array_equal(labels.cpu().numpy(), np_label_index(host, space.triple, space.col_of, ids, *ex.TRAIN_YEARS))
        assert labels.min().item() >= 0
    # no edge of the masked relation touches a seed (counted on the device tensors), and without the mask some do
    seed = torch.zeros(g[1].numel(), dtype=torch.bool, device=DEV)
    seed[x_ids] = True
    rel, rev = dgraph.edge_dict[space.triple[2]], dgraph.edge_dict["rev_" + space.triple[2]]
    at_seeds = lambda q: int((((q[4] == rel) & seed[q[3][1]]) | ((q[4] == rev) & seed[q[3][0]])).sum())
    plain = sample_subgraph_device(dgraph, ex.TRAIN_YEARS[1], TC.DEPTH, TC.WIDTH, TC.paper_seeds(ex, space), seed=TC.SAMPLE_SEED, plan=False)
    assert torch.equal(plain[1], g[1]) and at_seeds(g) == 0 and at_seeds(plain) > 0
    # the step
    node_rep = gnn(g[0], g[1], g[2], g[3], g[4])
    node_rep.retain_grad()
    res = head(node_rep[x_ids])
    loss = torch.nn.KLDivLoss(reduction="batchmean")(res, labels) if kind == "field" else torch.nn.functional.nll_loss(res, labels)
    loss.backward()
    torch.cuda.synchronize()
    P = TS.params_of(gnn, head, "head.")
    with torch.no_grad():
        terms = TS.kl_terms(res, labels) if kind == "field" else TS.nll_terms(res, labels)
    _isolation(kind, P, node_rep, batch, res, terms, tag)
    gnn.eval(), head.eval()
    with torch.no_grad():
        rep_inf = gnn(g[0], g[1], g[2], g[3], g[4])
        _isolation(kind, P, rep_inf, batch, head(rep_inf[x_ids]), None, tag + " / inference path")
    gnn.train(), head.train()
    step = _gradients(kind, gnn, head, node_rep, P, batch, T, R, tag)
    print("%s: loss %.6f, float64 %.6f" % (tag, loss.item(), step["loss"].item()))
    kw = {"labels": labels} if kind == "field" else {"index": labels}
    ndcg, rr = rank_metrics(res.detach(), **kw)
    want_ndcg, want_rr = np_rank_metrics(res.detach().cpu().numpy(), **{k: v.cpu().numpy() for k, v in kw.items()})
    assert np.array_equal(rr.cpu().numpy(), want_rr) and np.abs(ndcg.cpu().numpy() - want_ndcg).max() <= NDCG_TOL
    print("%s: %.2f s" % (tag, time.perf_counter() - t0))
