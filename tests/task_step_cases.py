"""What tests/test_task_steps.py (CPU) and tests/test_task_steps_gpu.py share: the shapes of the three task steps, their seeds and
hand-made candidate lists, the host copy of a batch, and the gradient rules.  Not a test module and not a conftest.

Gradient rules, per named tensor, against the float64 gradient `ref` of oracle.task_steps.task_step:

  zero        ref is exactly zero everywhere (a parameter of a type whose rows the loss never reads): the gradient under test is None
              or exactly zero.
  ordinary    `_grads_close(name, got, ref, rtol=5e-4)` of tests/test_backward_gpu.py, with its per-entry bound.
  cancelling  max |ref| below 1e-9 of the step's largest gradient entry without being identically zero: the terms of the sum cancel by
              algebra, so a relative bound on the result means nothing.  max |got| <= 5e-4 * S, where S is the magnitude of what is
              summed: the largest column of sum_rows |d loss / d node_rep| over the rows of the tensor's type (times sigmoid(skip) of
              that type for an a_linears bias); for the Matcher's left bias the rows are those of d loss / d left_linear(rep[author_key]),
              one per pair.  Which tensors are in this class is pinned by name (CANCELLING).

No tensor is left out; `emb.emb.weight` is skipped only when the module under test keeps no gradient for it."""
import importlib.util
import os
import re

import numpy as np
import torch

from pyhgt_amd import LabelSpace, candidate_pairs, seed_edge_mask
from test_backward_gpu import _grads_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_DIM, N_HID, N_HEADS, N_LAYERS = 48, 64, 4, 2
N_PAPER, DEPTH, WIDTH = 2000, 2, 8
SAMPLE_SEED, WEIGHT_SEED, HEAD_SEED = 11, 5, 3
# both sides of the wavefront / workgroup line of the loss kernels (64 | 65) and of their block of 256
AUTHOR_SIZES = [2, 3, 7, 63, 64, 65, 130, 257, 2, 64]
N_AUTHOR_SEEDS = 300
N_PAPER_SEEDS, N_FIELDS = 48, 65
GRAD_RTOL, CANCEL_BELOW = 5e-4, 1e-9
# The cancelling tensors of the author step.  Within a segment the paper is fixed, so the paper's projection ty and with it
# d score / d tx = ty / sqrt(n_hid) and d score / d h_author = W_l^T ty / sqrt(n_hid) are the same vectors for every candidate of the
# segment, and sum_segment d loss / d score = 0 (softmax minus one-hot).  So every segment's contribution cancels in
#   - the bias of the Matcher's left_linear: the column sum of d loss / d tx over the pairs, and
#   - the LayerNorm bias of the author type in the last layer: the column sum of d loss / d node_rep over the author rows.
# The paper steps have no such tensor.
CANCELLING = {"author": {"gcs.%d.base_conv.norms.1.bias" % (N_LAYERS - 1), "matcher.left_linear.bias"}, "field": set(), "venue": set()}
PREFIX = {"author": "matcher.", "field": "head.", "venue": "head."}
FIELD_LABEL, VENUE_LABEL = ("paper", "field", "PF_in_L2"), ("paper", "venue", "PV_Journal")


def example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------------------- the three batches
def author_graph(device):
    ex = example("train_author_disambiguation_device")
    dgraph, groups, first, year = ex.task_graph(N_PAPER, IN_DIM, device)
    return ex, dgraph, first, year


def author_seeds(ex, dgraph, first, year):
    """10 papers of the training years and 300 authors (the papers' first authors among them, the authors' seed time at the window's
    end) -> (inp, name_label): hand-made candidate lists of AUTHOR_SIZES serials, the true author first, the rest drawn without
    replacement, so that authors recur across lists and every paper row is gathered `size` times"""
    rng = np.random.default_rng(7)
    lo, hi = ex.TRAIN_YEARS
    papers = rng.choice(np.flatnonzero((year >= lo) & (year <= hi)), size=len(AUTHOR_SIZES), replace=False)
    true = first[papers]
    n_author = dgraph.n_nodes[dgraph.types.index("author")]
    others = rng.permutation(np.setdiff1d(np.arange(n_author), true))
    authors = rng.permutation(np.concatenate([np.unique(true), others])[:N_AUTHOR_SEEDS])
    serial = {int(a): i for i, a in enumerate(authors)}
    name_label = []
    for p, size in zip(papers, AUTHOR_SIZES):
        t = serial[int(first[p])]
        rest = rng.choice(np.setdiff1d(np.arange(N_AUTHOR_SEEDS), [t]), size=size - 1, replace=False)
        name_label.append([t] + rest.tolist())
    inp = {"paper": np.stack([papers, year[papers]], axis=1), "author": np.stack([authors, np.full(authors.size, hi)], axis=1)}
    return inp, name_label


def author_mask(ex, dgraph):
    return seed_edge_mask(dgraph, [ex.LABEL[2], "rev_" + ex.LABEL[2]], "paper", len(AUTHOR_SIZES))


def np_author_keys(paper_rows, author_rows, name_label):
    """the loop of the script (train_author_disambiguation.py:280-289) on host copies of the seeds' rows"""
    paper_key, author_key, key_size = [], [], []
    for i, serials in enumerate(name_label):
        paper_key += [np.repeat(paper_rows[i], len(serials))]
        author_key += [author_rows[np.asarray(serials)]]
        key_size += [len(serials)]
    return np.concatenate(paper_key), np.concatenate(author_key), np.asarray(key_size)


def paper_graph(device):
    ex = example("train_task_device_sampler")
    dgraph, n_nodes = ex.task_graph(N_PAPER, IN_DIM, device)
    return ex, dgraph, n_nodes


def paper_space(kind, dgraph, n_nodes):
    """field: 65 of the fields, a paper has several (PF_in_L2); venue: every venue a class, a paper has one journal"""
    if kind == "field":
        return LabelSpace(dgraph, FIELD_LABEL, np.random.default_rng(9).choice(n_nodes["field"], N_FIELDS, replace=False))
    return LabelSpace(dgraph, VENUE_LABEL, np.arange(n_nodes["venue"]))


def paper_seeds(ex, space):
    """48 papers with at least one label in the training years, each at the time of its first label edge"""
    ids, years = space.targets(*ex.TRAIN_YEARS)
    pick = np.random.default_rng(13).choice(ids.size, size=N_PAPER_SEEDS, replace=False)
    return {"paper": np.stack([ids[pick], years[pick]], axis=1)}


def paper_mask(space, dgraph):
    return seed_edge_mask(dgraph, [space.triple[2], "rev_" + space.triple[2]], "paper", N_PAPER_SEEDS)


def host_batch(g, **more):
    """the five tensors of a sampled batch that GNN.forward takes, on the host, plus the keys or labels of the step"""
    batch = {k: g[i].detach().cpu() for i, k in enumerate(("x", "node_type", "edge_time", "edge_index", "edge_type"))}
    batch.update({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in more.items()})
    return batch


def host_author_batch(sample, ex, dgraph, first, year):
    """the author batch through `sample` (sample_subgraph_host or sample_subgraph_device) -> (g, batch on the host, name_label, the keys
    of candidate_pairs where g lives)"""
    inp, name_label = author_seeds(ex, dgraph, first, year)
    g = sample(dgraph, ex.TRAIN_YEARS[1], DEPTH, WIDTH, inp, seed=SAMPLE_SEED, mask=author_mask(ex, dgraph))
    paper_key, author_key, sizes = candidate_pairs(g, name_label)
    return g, host_batch(g, paper_key=paper_key, author_key=author_key, sizes=sizes), name_label, (paper_key, author_key, sizes)


def host_paper_batch(sample, kind, ex, dgraph, n_nodes):
    """a paper batch through `sample` -> (g, batch on the host, the LabelSpace, the labels where g lives)"""
    space = paper_space(kind, dgraph, n_nodes)
    g = sample(dgraph, ex.TRAIN_YEARS[1], DEPTH, WIDTH, paper_seeds(ex, space), seed=SAMPLE_SEED, mask=paper_mask(space, dgraph))
    ids = g.indxs["paper"][:N_PAPER_SEEDS]
    labels = {"ylabel": space.distribution(ids, *ex.TRAIN_YEARS)} if kind == "field" else {"y": space.index(ids, *ex.TRAIN_YEARS)}
    return g, host_batch(g, rows=g.seed_rows("paper"), **labels), space, next(iter(labels.values()))


# ---------------------------------------------------------------------------------------------------------------- the gradient rules
def gradient_classes(ref_grads):
    """-> (names whose float64 gradient is exactly zero, names of the cancelling class, the step's largest gradient entry)"""
    top = max(g.abs().max().item() for g in ref_grads.values())
    zero = {k for k, g in ref_grads.items() if not g.any()}
    cancelling = {k for k, g in ref_grads.items() if k not in zero and g.abs().max().item() < CANCEL_BELOW * top}
    return zero, cancelling, top


def cancelling_scale(name, step, P, node_type):
    """S of the module docstring for a last-layer `norms.<t>.bias` or `a_linears.<t>.bias`, or the Matcher's left bias"""
    if name == "matcher.left_linear.bias":
        return step["grad_left"].abs().sum(dim=0).max().item()
    m = re.fullmatch(r"gcs\.(\d+)\.base_conv\.(norms|a_linears)\.(\d+)\.bias", name)
    assert m and int(m.group(1)) == N_LAYERS - 1, "%s: no scale is defined for a cancelling tensor of this kind" % name
    t = int(m.group(3))
    S = step["grad_rep"][node_type == t].abs().sum(dim=0).max().item()
    if m.group(2) == "a_linears":
        S *= torch.sigmoid(P["gcs.%d.base_conv.skip" % (N_LAYERS - 1)].detach().double()[t]).item()
    return S


def check_gradient_rules(kind, got, step, P, node_type, tag):
    """got: {name: gradient tensor or None} for every name of step["grads"].  Asserts every rule and returns the worst error per class
    (ordinary: of the tensor's largest entry; cancelling: of S)."""
    zero, cancelling, top = gradient_classes(step["grads"])
    assert cancelling == CANCELLING[kind], (kind, sorted(cancelling))
    assert set(got) == set(step["grads"])
    worst, count = {"ordinary": 0.0, "cancelling": 0.0}, {"zero": 0, "ordinary": 0, "cancelling": 0, "skipped": 0}
    for name, ref in step["grads"].items():
        g = got[name]
        if name.endswith("emb.emb.weight") and g is None:
            count["skipped"] += 1
            continue
        if name in zero:
            assert g is None or not g.detach().cpu().any(), "%s: the float64 gradient is exactly zero, this one is not" % name
            count["zero"] += 1
        elif name in cancelling:
            S = cancelling_scale(name, step, P, node_type)
            err = g.detach().cpu().double().abs().max().item() / S
            assert err <= GRAD_RTOL, "%s: %.3e of S = %.3e; the terms cancel (float64: %.1e of S)" % (name, err, S, ref.abs().max().item() / S)
            worst["cancelling"] = max(worst["cancelling"], err)
            count["cancelling"] += 1
        else:
            assert g is not None, name
            worst["ordinary"] = max(worst["ordinary"], _grads_close(name, g, ref, rtol=GRAD_RTOL))
            count["ordinary"] += 1
    print("%s: gradients of %d tensors: %d exactly zero, %d ordinary, worst %.2e of the largest entry, %d cancelling, worst %.2e of S, "
          "%d skipped; largest entry of the step %.3e" % (tag, len(got), count["zero"], count["ordinary"], worst["ordinary"],
                                                         count["cancelling"], worst["cancelling"], count["skipped"], top))
    return worst
