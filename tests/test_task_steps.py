"""The float64 task steps of oracle/task_steps.py on the CPU: its heads against the verbatim reference modules, which gradient falls in
which class of the gradient rules (tests/task_step_cases.py) on host-sampled batches, and the same steps in float32 under those rules --
what a correct single-precision implementation gives, so the rules are satisfiable with nothing left out.  tests/test_task_steps_gpu.py
applies the same rules to the device."""
import math
import time

import numpy as np
import pytest
import torch

import task_step_cases as TC
from oracle import hgt_oracle as O
from oracle import task_steps as TS
from oracle.reference_loader import reference_available
from pyhgt_amd import np_pair_rank_loss, sample_subgraph_host

AUTHOR_TYPE = 1
CANCELLING_NAME = "gcs.%d.base_conv.norms.%d.bias" % (TC.N_LAYERS - 1, AUTHOR_TYPE)


def _head_params(kind, n_out=None):
    g = torch.Generator().manual_seed(TC.HEAD_SEED)
    b = 1.0 / math.sqrt(TC.N_HID)
    uni = lambda *shape: (torch.rand(shape, generator=g) * 2 - 1) * b
    if kind == "author":
        return {"matcher.left_linear.weight": uni(TC.N_HID, TC.N_HID), "matcher.left_linear.bias": uni(TC.N_HID),
                "matcher.right_linear.weight": uni(TC.N_HID, TC.N_HID), "matcher.right_linear.bias": uni(TC.N_HID)}
    return {"head.linear.weight": uni(n_out, TC.N_HID), "head.linear.bias": uni(n_out)}


@pytest.fixture(scope="module")
def steps():
    """per kind (batch, parameters, T, R, the float64 step): computed once, read by every test, changed by none"""
    out = {}
    ex, dgraph, first, year = TC.author_graph(None)
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    assert dgraph.types[AUTHOR_TYPE] == "author"
    _, batch, _, _ = TC.host_author_batch(sample_subgraph_host, ex, dgraph, first, year)
    out["author"] = (batch, _head_params("author"))
    ex, dgraph, n_nodes = TC.paper_graph(None)
    for kind in ("field", "venue"):
        _, batch, space, _ = TC.host_paper_batch(sample_subgraph_host, kind, ex, dgraph, n_nodes)
        out[kind] = (batch, _head_params(kind, space.n_cols))
    sd = O.make_gnn_state_dict(TC.IN_DIM, TC.N_HID, T, R, TC.N_HEADS, TC.N_LAYERS, True, True, True, seed=TC.WEIGHT_SEED)
    res = {}
    for kind, (batch, head) in out.items():
        P = dict(sd, **head)
        t0 = time.perf_counter()
        step = TS.task_step(kind, P, batch, T, R, TC.N_HEADS, TC.N_LAYERS)
        print("%s step in float64: %d nodes, %d edges, %d loss rows, loss %.6f, %.2f s" % (
            kind, batch["x"].shape[0], batch["edge_type"].numel(), step["terms"].numel(), step["loss"].item(), time.perf_counter() - t0))
        res[kind] = (batch, P, T, R, step)
    return res


@pytest.mark.skipif(not reference_available(), reason="the reference tree is not present")
def test_heads_equal_the_reference_modules_in_float64():
    from oracle.reference_loader import load_reference_model
    ref = load_reference_model()
    g = torch.Generator().manual_seed(1)
    rep = torch.randn(90, TC.N_HID, generator=g, dtype=torch.float64)
    a_key, p_key = torch.randint(0, 90, (200,), generator=g), torch.randint(0, 90, (200,), generator=g)
    gout = torch.randn(200, generator=g, dtype=torch.float64)
    matcher = ref.Matcher(TC.N_HID).double()
    P = {"matcher." + k: v.detach() for k, v in matcher.named_parameters()}
    a, b = rep.clone().requires_grad_(True), rep.clone().requires_grad_(True)
    want = matcher(a[a_key], a[p_key], pair=True)
    got = TS.matcher_pair(P, b, a_key, p_key)
    (want * gout).sum().backward()
    (got * gout).sum().backward()
    assert (got - want).abs().max().item() <= 1e-12 and (a.grad - b.grad).abs().max().item() <= 1e-12
    head = ref.Classifier(TC.N_HID, 65).double()
    P = {"head." + k: v.detach() for k, v in head.named_parameters()}
    gout = torch.randn(40, 65, generator=g, dtype=torch.float64)
    a, b = rep.clone().requires_grad_(True), rep.clone().requires_grad_(True)
    want, got = head(a[:40]), TS.classifier(P, b[:40])
    (want * gout).sum().backward()
    (got * gout).sum().backward()
    assert (got - want).abs().max().item() <= 1e-12 and (a.grad - b.grad).abs().max().item() <= 1e-12


def test_mask_softmax_is_the_pair_rank_loss_rule():
    """np_pair_rank_loss is the positive loss and its gradient (d loss / d scores with g = 1); mask_softmax returns that loss"""
    sizes = TC.AUTHOR_SIZES
    x = torch.from_numpy(np.random.default_rng(2).uniform(-8, 8, size=sum(sizes))).requires_grad_(True)
    loss = TS.mask_softmax(x, sizes)
    loss.backward()
    want, grad = np_pair_rank_loss(x.detach().numpy(), sizes, return_grad=True)
    assert want > 0 and abs(loss.item() - want) <= 1e-12 * want
    assert np.abs(x.grad.numpy() - grad).max() <= 1e-12
    assert abs(TS.mask_softmax_terms(x, sizes).sum().item() - want) <= 1e-12 * want


def test_gradient_classes_of_the_author_step(steps):
    batch, P, T, R, step = steps["author"]
    assert batch["sizes"].tolist() == TC.AUTHOR_SIZES and batch["paper_key"].numel() == sum(TC.AUTHOR_SIZES) == 657
    zero, cancelling, top = TC.gradient_classes(step["grads"])
    last = "gcs.%d.base_conv." % (TC.N_LAYERS - 1)
    for t in range(T):
        if t in (0, AUTHOR_TYPE):                                        # paper, author: the only rows the loss reads
            continue
        for name in ["q_linears.%d.weight", "q_linears.%d.bias", "a_linears.%d.weight", "a_linears.%d.bias", "norms.%d.weight", "norms.%d.bias"]:
            assert last + name % t in zero, name % t
        assert step["grads"][last + "skip"][t].item() == 0.0
    assert step["grads"][last + "skip"][0].item() != 0.0 and step["grads"][last + "skip"][AUTHOR_TYPE].item() != 0.0
    S = TC.cancelling_scale(CANCELLING_NAME, step, P, batch["node_type"])
    small = step["grads"][CANCELLING_NAME].abs().max().item()
    print("author step: %d tensors exactly zero: %s; %s = %.2e = %.1e of S = %.3e; largest entry of the step %.3e"
          % (len(zero), sorted(zero), CANCELLING_NAME, small, small / S, S, top))
    assert small < 1e-12 * S
    S_left = TC.cancelling_scale("matcher.left_linear.bias", step, P, batch["node_type"])
    small = step["grads"]["matcher.left_linear.bias"].abs().max().item()
    print("author step: matcher.left_linear.bias = %.2e = %.1e of S = %.3e" % (small, small / S_left, S_left))
    assert small < 1e-12 * S_left
    # and no other tensor is below 1e-9 of the largest entry
    assert cancelling == {CANCELLING_NAME, "matcher.left_linear.bias"} == TC.CANCELLING["author"]


@pytest.mark.parametrize("kind", ["field", "venue"])
def test_gradient_classes_of_the_paper_steps(steps, kind):
    batch, P, T, R, step = steps[kind]
    zero, cancelling, top = TC.gradient_classes(step["grads"])
    last = "gcs.%d.base_conv." % (TC.N_LAYERS - 1)
    for t in range(1, T):                                                # only paper rows are read
        for name in ["q_linears.%d.weight", "a_linears.%d.bias", "norms.%d.weight", "norms.%d.bias"]:
            assert last + name % t in zero, name % t
    assert cancelling == TC.CANCELLING[kind] == set()
    if kind == "field":
        assert batch["ylabel"].shape == (TC.N_PAPER_SEEDS, TC.N_FIELDS) and (batch["ylabel"] > 0).sum(1).max() > 1
        assert (batch["ylabel"].double().sum(1) - 1).abs().max() < 1e-6
    else:
        assert batch["y"].min() >= 0


@pytest.mark.parametrize("kind", TS.KINDS)
def test_float32_step_stays_within_the_gradient_rules(steps, kind):
    batch, P, T, R, step = steps[kind]
    f32 = TS.task_step(kind, P, batch, T, R, TC.N_HEADS, TC.N_LAYERS, dtype=torch.float32)
    assert all(g.dtype == torch.float32 for g in f32["grads"].values())
    print("%s step in float32: node_rep max err %.2e, loss err %.2e" % (kind, (f32["rep"].double() - step["rep"]).abs().max().item(),
                                                                         abs(f32["loss"].item() - step["loss"].item())))
    TC.check_gradient_rules(kind, dict(f32["grads"]), step, P, batch["node_type"], "float32 %s step" % kind)
    for name in sorted(TC.CANCELLING[kind]):                             # the cancelling-tensor rule gates: 1e-2 * S does not pass
        S = TC.cancelling_scale(name, step, P, batch["node_type"])
        off = dict(f32["grads"])
        off[name] = off[name] + 1e-2 * S
        with pytest.raises(AssertionError, match="%s.*the terms cancel" % name):
            TC.check_gradient_rules(kind, off, step, P, batch["node_type"], "perturbed")
