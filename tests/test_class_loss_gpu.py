"""The classification-loss kernels (csrc/hgt_task_loss.hip) and the label lists (csrc/hgt_sampler_labels.hip) on the GPU against the
rules of pyhgt_amd/metrics.py and pyhgt_amd/sampler.py on the same inputs.

Gates (derived, not chosen; float32 device results against the float64 rule):
  terms      per row 4 x max(E_torch, 2^-23 sum_j |summand_j|): E_torch is the error of torch's own float32 CPU chain (log_softmax +
             nll_loss / kl_div) on the same inputs against float64 -- another summation order is as legitimate as torch's -- and the
             floor keeps rows alive on which torch happens to be exact.  The summands are the quantities that are added up, each
             with its own float32 rounding: l_j log l_j and l_j logp_j (a list: log c and logp_col / c).  They are not paired
             off first: where a prediction equals its label, l_j (log l_j - logp_j) is 0 in exact arithmetic, while log l_j and a
             float32 logp_j still differ by their roundings -- the device scored such a row 1.9e-09 where torch's chain, whose
             float32 log 0.5 and -log 2 cancel, gave exactly 0
  gradients  per element 4 x max(largest error of torch's float32 gradient in that row, 2^-23 max(W, 1))
Measured on an MI355X (pytest -s prints them): the worst term error over every case of the first test was 7.9e-06 under a gate of
4.1e-05 there, the worst gradient error 1.3e-07 under 5.1e-07.  Classifier.loss, worst of the four cases: loss 4.1e-07 under 6.9e-07,
x 4.1e-09 under 1.0e-08, weight 2.1e-08 under 8.4e-08, bias 2.3e-08 under 2.6e-08 (the column sums of the existing deterministic
weight-gradient path: torch's float32 sum of 64 rows is nearly correctly rounded, so four times its error is about 1.7 ulp of a sum)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import test_class_loss as CL
from oracle import task_steps as TS
from pyhgt_amd import _lib, Classifier, LabelSpace, class_loss, np_class_loss, np_label_columns, np_label_counts, np_label_distribution, \
    np_label_index

pytestmark = pytest.mark.gpu

ROOT = CL.ROOT
DEV = "cuda:0"
W = _lib.CLASS_LOSS_WAVE_COLS
EPS32 = 2.0 ** -23
SIZES = [1, 2, 63, 64, 65, W - 1, W, W + 1, 1023, 1024, 1025, 4099, 20011]
WORST = {"term": (0.0, 0.0), "grad": (0.0, 0.0)}


def place(a, layout, fill=float("nan")):
    """a host array [n, C] on the device: contiguous, or the columns 1 .. C + 1 of a tensor three columns wider whose other columns
    hold `fill` (an odd first column: rows that are not 16-byte aligned; NaN guards on both sides)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if layout == "contiguous":
        return t.to(DEV)
    wide = torch.full((a.shape[0], a.shape[1] + 3), fill, dtype=t.dtype)
    wide[:, 1:1 + a.shape[1]] = t
    view = wide.to(DEV)[:, 1:1 + a.shape[1]]
    assert view.data_ptr() % 16 == 4
    return view


def torch32_chain(x32, dense32=None, index=None):
    """(terms, gradient) of torch's float32 CPU chain as float64 arrays"""
    return CL.torch_chain(x32, labels=dense32, index=index, dtype=torch.float32)


def gates(x32, dense, index=None):
    """-> (want terms, want grad, term gate [n], gradient gate [n, 1]) for valid rows; dense: the float32 labels the device form stands for"""
    want, want_grad = np_class_loss(x32, labels=dense.astype(np.float64), return_grad=True) if index is None else \
        np_class_loss(x32, index=index, return_grad=True)
    t32, g32 = torch32_chain(x32, dense, index) if index is None else torch32_chain(x32, index=index)
    x = x32.astype(np.float64)
    with np.errstate(all="ignore"):
        m = x.max(1, keepdims=True)
        logp = x - m - np.log(np.exp(x - m).sum(1, keepdims=True))
        l = dense.astype(np.float64)
        summands = np.where(l > 0, np.abs(l * np.log(l)) + np.abs(l * logp), 0.0).sum(1)
    # (fmax: torch's kl_div forms 0 * -inf = NaN on a row with -inf off its labels; the floor alone gates such a row)
    term_gate = 4 * np.fmax(np.abs(t32 - want), EPS32 * summands)
    grad_gate = 4 * np.fmax(np.abs(g32 - want_grad).max(1), EPS32 * np.maximum(l.sum(1), 1.0))[:, None]
    return want, want_grad, term_gate, grad_gate


def device_terms(x, **kw):
    """-> (terms, gradient of their sum) as float64 host arrays, through the autograd wrapper"""
    leaf = x.detach().requires_grad_()
    terms = class_loss(leaf, reduce=None, **kw)
    assert terms.dtype == torch.float32 and terms.shape == (x.shape[0],) and terms.device == x.device
    terms.sum().backward()
    return terms.detach().cpu().numpy().astype(np.float64), leaf.grad.cpu().numpy().astype(np.float64)


def agree(x32, layout, dense, what, **kw_host):
    """one device call, forward and backward, against the rule under the gates of the module docstring"""
    index = kw_host.get("index")
    want, want_grad, term_gate, grad_gate = gates(x32, dense, index)
    kw = {k: place(v, layout) if k == "labels" else torch.from_numpy(np.asarray(v)).to(DEV) for k, v in kw_host.items()}
    terms, grad = device_terms(place(x32, layout), **kw)
    assert np.isfinite(terms).all() and np.isfinite(grad).all()
    err, gerr = np.abs(terms - want), np.abs(grad - want_grad)
    r, (gr, gc) = err.argmax(), np.unravel_index((gerr / grad_gate).argmax(), gerr.shape)
    print("C=%d n=%d %s %s: term error %.3e (gate %.3e), gradient error %.3e (gate %.3e)"
          % (x32.shape[1], x32.shape[0], layout, what, err[r], term_gate[r], gerr[gr, gc], grad_gate[gr, 0]))
    if err[r] > WORST["term"][0]:
        WORST["term"] = (err[r], term_gate[r])
    if gerr[gr, gc] > WORST["grad"][0]:
        WORST["grad"] = (gerr[gr, gc], grad_gate[gr, 0])
    assert (err <= term_gate).all() and (gerr <= grad_gate).all()
    return terms, grad


def case(c, n, seed):
    """float32 logits [n, C] as test_class_loss makes them, dense labels (1, 3, C non-zeros, an all-zero row), an index per row"""
    rng = np.random.default_rng(seed)
    x = CL.make_logits(rng, n, c).astype(np.float32)
    dense = CL.make_dense(rng, n, c).astype(np.float32)
    return rng, x, dense, rng.integers(0, c, size=n)


@pytest.mark.parametrize("layout", ["contiguous", "odd slice"])
@pytest.mark.parametrize("c", SIZES)
def test_terms_and_gradients_of_all_three_label_forms(c, layout):
    for n in (1, 5):
        rng, x, dense, index = case(c, n, 1000 * c + n)
        agree(x, layout, CL.dense_of(c, index=index).astype(np.float32), "index", index=index)
        agree(x, layout, dense, "dense", labels=dense)
        for width in (1, 8, 300):
            cols = CL.make_columns(rng, n, c, width).astype(np.int32)
            count = (cols >= 0).sum(1).astype(np.int32)
            terms, grad = agree(x, layout, CL.dense_of(c, columns=cols).astype(np.float32), "columns/%d" % width, columns=cols, count=count)
            assert (terms[count == 0] == 0).all() and not grad[count == 0].any()
        if n == 5 and c > 3:
            # -inf on every unlabelled column of the row with three labels: a finite term, gradient 0 there
            x[1, dense[1] == 0] = -np.inf
            terms, grad = agree(x, layout, dense, "dense, -inf off the labels", labels=dense)
            assert not grad[1, dense[1] == 0].any() and terms[3] == 0 and not grad[3].any()
            cols = np.full((n, 8), -1, np.int32)
            cols[:, 0] = index
            cols[1, :3] = np.flatnonzero(dense[1])
            agree(x, layout, CL.dense_of(c, columns=cols).astype(np.float32), "columns, -inf off the labels", columns=cols)
    print("worst so far: term %.3e under %.3e, gradient %.3e under %.3e" % (WORST["term"] + WORST["grad"]))


# ---------------------------------------------------------------------------------------------------------------- the C ABI, directly
def raw(x, ld, n_cols, labels=None, ld_labels=0, index=None, columns=None, count=None, grad=None, ld_grad=0, grad_loss=None):
    """hgt_class_loss and, with `grad`, hgt_class_loss_bwd on device tensors as they are -> (loss, lse, wsum)"""
    lib, n = _lib.load(), x.shape[0]
    ptr = lambda t: None if t is None else t.data_ptr()
    loss, lse, wsum = torch.empty(n, device=DEV), torch.empty(n, 2, device=DEV), torch.empty(n, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    head = (ptr(x), ld, n, n_cols, ptr(labels), ld_labels, ptr(index), ptr(columns), 0 if columns is None else columns.shape[1], ptr(count))
    _lib.check(lib.hgt_class_loss(*head, ptr(loss), ptr(lse), ptr(wsum), st), "hgt_class_loss")
    if grad is not None:
        _lib.check(lib.hgt_class_loss_bwd(*head, ptr(lse), ptr(wsum), ptr(grad_loss), ptr(grad), ld_grad, st), "hgt_class_loss_bwd")
    torch.cuda.synchronize()
    return loss, lse, wsum


@pytest.mark.parametrize("c", [5, 64, W, W + 1, 1025])
def test_guard_columns(c):
    """logits, labels and the gradient padded to ld = C + 3 with NaN / a poison value in the padding: nothing turns NaN and the padding
    of the gradient survives"""
    n, ld = 5, c + 3
    rng, x, dense, index = case(c, n, 50 + c)
    xw = torch.full((n, ld), float("nan"), device=DEV)
    lw = torch.full((n, ld), float("nan"), device=DEV)
    xw[:, :c], lw[:, :c] = torch.from_numpy(x).to(DEV), torch.from_numpy(dense).to(DEV)
    g = torch.from_numpy(rng.uniform(0.5, 2.0, size=n).astype(np.float32)).to(DEV)
    cols = torch.from_numpy(CL.make_columns(rng, n, c, 8).astype(np.int32)).to(DEV)
    for kw in ({"labels": lw, "ld_labels": ld}, {"index": torch.from_numpy(index).to(DEV)}, {"columns": cols}):
        grad = torch.full((n, ld), -7.25, device=DEV)
        loss, lse, wsum = raw(xw, ld, c, grad=grad, ld_grad=ld, grad_loss=g, **kw)
        assert torch.isfinite(loss).all() and torch.isfinite(lse).all() and torch.isfinite(wsum).all()
        assert torch.isfinite(grad[:, :c]).all() and (grad[:, c:] == -7.25).all()
        host = {k: v.cpu().numpy()[:, :c] if k == "labels" else v.cpu().numpy() for k, v in kw.items() if k != "ld_labels"}
        want, want_grad = np_class_loss(x, return_grad=True, **host)
        assert np.allclose(loss.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
        assert np.allclose(grad[:, :c].cpu().numpy(), want_grad * g.cpu().numpy()[:, None], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("c", [7, W, 1500])
def test_special_rows(c):
    rng, x, dense, _ = case(c, 6, 70 + c)
    xd = torch.from_numpy(x).to(DEV)
    # index: -1 rows are ignored, index = C is NaN in that row only
    index = np.array([-1, 2, c, -100, c - 1, 0])
    terms, grad = device_terms(xd, index=torch.from_numpy(index).to(DEV))
    want, want_grad = np_class_loss(x, index=index, return_grad=True)
    assert np.array_equal(np.isnan(terms), np.isnan(want)) and np.isnan(terms).tolist() == [False, False, True, False, False, False]
    assert terms[0] == 0 and terms[3] == 0 and not grad[0].any() and not grad[3].any() and np.isnan(grad[2]).all()
    ok = [1, 4, 5]
    assert np.isfinite(grad[ok]).all() and np.allclose(terms[ok], want[ok], rtol=1e-5, atol=1e-6) and np.allclose(grad[ok], want_grad[ok], atol=1e-6)
    # columns: a column = C and count > width are NaN in their rows only; an empty list is 0
    cols = np.full((6, 4), -1, np.int32)
    cols[0, :2], cols[1, :3], cols[2, 0], cols[4, :4], cols[5, 1] = [1, c], [0, 2, 3], 1, [0, 1, 2, 3], c - 1
    count = np.array([2, 3, 1, 0, 5, 1], np.int32)
    terms, grad = device_terms(xd, columns=torch.from_numpy(cols).to(DEV), count=torch.from_numpy(count).to(DEV))
    want, want_grad = np_class_loss(x, columns=cols, count=count, return_grad=True)
    assert np.isnan(terms).tolist() == np.isnan(want).tolist() == [True, False, False, False, True, False]
    assert np.isnan(grad[[0, 4]]).all() and terms[3] == 0 and not grad[3].any()
    ok = [1, 2, 5]
    assert np.allclose(terms[ok], want[ok], rtol=1e-5, atol=1e-6) and np.allclose(grad[ok], want_grad[ok], atol=1e-6)
    terms = device_terms(xd, columns=torch.from_numpy(cols).to(DEV))[0]          # without the counts the full list of row 4 is scored
    assert np.isnan(terms).tolist() == [True, False, False, False, False, False]
    # dense: a negative or a NaN entry
    dense[0, 0], dense[2, c - 1] = -0.25, np.nan
    terms, grad = device_terms(xd, labels=torch.from_numpy(dense).to(DEV))
    assert np.isnan(terms).tolist() == [True, False, True, False, False, False] and np.isnan(grad[[0, 2]]).all()
    assert np.isfinite(grad[[1, 3, 4, 5]]).all()


@pytest.mark.parametrize("c", [64, W, W + 1, 4099])
def test_a_rows_bits_depend_on_the_row_alone(c):
    """row r of a 5-row call equals its 1-row call -- in place and as an aligned copy -- bit for bit, and two calls give equal bits"""
    rng, x, dense, index = case(c, 5, 90 + c)
    cols = CL.make_columns(rng, 5, c, 8).astype(np.int32)
    forms = {"index": torch.from_numpy(index), "labels": torch.from_numpy(dense), "columns": torch.from_numpy(cols)}
    for layout in ("contiguous", "odd slice"):
        xd = place(x, layout)
        for name, lab in forms.items():
            lab = lab.to(DEV)
            bits = lambda pair: [a.view(np.uint64) for a in pair]
            whole = bits(device_terms(xd, **{name: lab}))
            again = bits(device_terms(xd, **{name: lab}))
            assert np.array_equal(whole[0], again[0]) and np.array_equal(whole[1], again[1])
            for r in range(5):
                for rows in (xd[r:r + 1], xd[r:r + 1].clone()):
                    one = bits(device_terms(rows, **{name: lab[r:r + 1]}))
                    assert np.array_equal(one[0][0], whole[0][r]) and np.array_equal(one[1][0], whole[1][r]), (layout, name, r)


@pytest.mark.parametrize("c", [40, 349])
def test_reduce_modes_against_torch_on_the_device(c):
    """NLLLoss() / KLDivLoss('batchmean') and their sums on torch.log_softmax of the same device logits.  Two float32 evaluations of the
    same sum: each term is within its gate of float64, and the two reductions round n partial sums each, so the difference is bounded by
    (2 sum_r gate_r + 2 n 2^-24 sum_r |term_r|) / divisor"""
    n = 37
    rng, x, dense, index = case(c, n, 200 + c)
    index[[3, 11]] = -100                                                         # torch's default ignore_index
    xd = torch.from_numpy(x).to(DEV)
    logp = torch.log_softmax(xd, dim=-1)
    cols = CL.make_columns(rng, n, c, 8).astype(np.int32)
    cdense = CL.dense_of(c, columns=cols).astype(np.float32)
    valid = index >= 0
    _, _, gate_i, _ = gates(x[valid], CL.dense_of(c, index=index[valid]).astype(np.float32), index[valid])
    for kw, lab, gate, den in (({"index": torch.from_numpy(index).to(DEV)}, None, gate_i, valid.sum()),
                               ({"labels": torch.from_numpy(dense).to(DEV)}, dense, gates(x, dense)[2], n),
                               ({"columns": torch.from_numpy(cols).to(DEV)}, cdense, gates(x, cdense)[2], n)):
        terms = class_loss(xd, reduce=None, **kw)
        bound = 2 * gate.sum() + 2 * n * 2.0 ** -24 * terms.abs().sum().item()
        if lab is None:
            want_sum = torch.nn.NLLLoss(reduction="sum")(logp, kw["index"]).item()
            want_mean = torch.nn.NLLLoss()(logp, kw["index"]).item()
        else:
            want_sum = torch.nn.KLDivLoss(reduction="sum")(logp, torch.from_numpy(lab).to(DEV)).item()
            want_mean = torch.nn.KLDivLoss(reduction="batchmean")(logp, torch.from_numpy(lab).to(DEV)).item()
        got_sum, got_mean = class_loss(xd, reduce="sum", **kw).item(), class_loss(xd, **kw).item()
        print("C=%d %s: sum %.3e off (bound %.3e), mean %.3e off" % (c, list(kw)[0], abs(got_sum - want_sum), bound, abs(got_mean - want_mean)))
        assert abs(got_sum - want_sum) <= bound and abs(got_mean - want_mean) <= bound / den
        assert got_sum == terms.sum().item()
    none = torch.full((4,), -1, device=DEV)
    assert torch.isnan(class_loss(xd[:4], index=none)) and class_loss(xd[:4], index=none, reduce="sum").item() == 0
    empty = class_loss(xd[:0].requires_grad_(), index=none[:0], reduce=None)
    assert empty.shape == (0,) and empty.requires_grad


# ---------------------------------------------------------------------------------------------------------------- label lists
@pytest.mark.parametrize("n_cols", [131072, 131073])
def test_label_space_columns_equal_the_numpy_sibling(n_cols):
    """one and two passes of the bitmap; rows with 0, 1, 5 and about 300 classes, classes on both sides of the line, repeated sources,
    ids outside the type; every width, with and without a window; and the outputs of hgt_sampler_labels as they were"""
    host, dev = CL.label_graph(), CL.label_graph(device=DEV)
    space, ids = LabelSpace(dev, ("a", "b", "ab"), np.arange(n_cols)), CL.LABEL_IDS
    for window in ((None, None), (3, 6)):
        for width in (None, 1, 4, 5, 299, 300, 1000):
            want = np_label_columns(host, space.triple, space.col_of, ids, *window, width=width)
            got = space.columns(torch.from_numpy(ids).to(DEV) if width == 4 else ids, *window, width=width)
            assert got[0].dtype == got[1].dtype == torch.int32 and got[0].device.type == "cuda"
            assert got[0].shape == want[0].shape and np.array_equal(got[0].cpu().numpy(), want[0]), (window, width)
            assert np.array_equal(got[1].cpu().numpy(), want[1])
        assert want[1].max() > 100
        dist, index, count = space.distribution(ids, *window), space.index(ids, *window), space.counts(ids, *window)
        assert np.array_equal(dist.cpu().numpy().view(np.uint32),
                              np_label_distribution(host, space.triple, space.col_of, n_cols, ids, *window).view(np.uint32))
        assert np.array_equal(index.cpu().numpy(), np_label_index(host, space.triple, space.col_of, ids, *window))
        assert np.array_equal(count.cpu().numpy(), np_label_counts(host, space.triple, space.col_of, ids, *window))
    cols, count = space.columns(np.zeros(0, np.int64), width=3)
    assert cols.shape == (0, 3) and count.shape == (0,) and space.columns(np.zeros(0, np.int64))[0].shape == (0, 1)


def test_label_lists_and_dense_labels_give_the_same_loss():
    host, dev = CL.label_graph(), CL.label_graph(device=DEV)
    n_cols = 131073
    space, ids = LabelSpace(dev, ("a", "b", "ab"), np.arange(n_cols)), CL.LABEL_IDS
    x = torch.from_numpy(np.random.default_rng(5).uniform(-5, 5, size=(ids.size, n_cols)).astype(np.float32)).to(DEV)
    cols, count = space.columns(ids)
    a = class_loss(x, columns=cols, count=count, reduce=None).cpu().numpy().astype(np.float64)
    dense = space.distribution(ids)
    b = class_loss(x, labels=dense, reduce=None).cpu().numpy().astype(np.float64)
    gate = gates(x.cpu().numpy(), dense.cpu().numpy())[2]
    assert (np.abs(a - b) <= 2 * gate).all() and (a[count.cpu().numpy() == 0] == 0).all()
    short = class_loss(x, columns=cols[:, :4].contiguous(), count=count, reduce=None).cpu().numpy()
    assert np.array_equal(np.isnan(short), count.cpu().numpy() > 4)             # a truncated list is never scored silently


# ---------------------------------------------------------------------------------------------------------------- Classifier.loss
@pytest.mark.parametrize("kind, n_out", [("venue", 40), ("field", 40), ("field", 349), ("venue", 349)])
def test_classifier_loss_against_the_float64_chain(kind, n_out):
    """loss and the gradients of x, weight and bias against oracle.task_steps.classifier + kl_terms / nll_terms in float64; the gate of
    a gradient is 4 x the largest error of the same chain in float32 on the CPU in that tensor, the gate of the loss 4 x the mean
    error of that chain's per-row terms"""
    n, n_hid = 64, 32
    rng = np.random.default_rng(n_out)
    torch.manual_seed(n_out)
    head = Classifier(n_hid, n_out, deterministic=True).to(DEV)
    x = torch.from_numpy(rng.standard_normal((n, n_hid)).astype(np.float32))
    cols = CL.make_columns(rng, n, n_out, 8).astype(np.int32)
    cols[cols[:, 0] < 0, 0] = 0                                                   # every row has a class: rows that sum to 1
    ylabel = torch.from_numpy(CL.dense_of(n_out, columns=cols).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, n_out, size=n))

    def chain(dtype):
        P = {"head." + k: v.detach().cpu().to(dtype).requires_grad_() for k, v in head.named_parameters()}
        xx = x.clone().to(dtype).requires_grad_()
        logp = TS.classifier(P, xx)
        terms = TS.kl_terms(logp, ylabel) if kind == "field" else TS.nll_terms(logp, y)
        loss = terms.sum() / n
        grads = torch.autograd.grad(loss, [xx, P["head.linear.weight"], P["head.linear.bias"]])
        return [loss.detach().double()] + [g.double() for g in grads] + [terms.detach().double()]

    want, f32 = chain(torch.float64), chain(torch.float32)
    loss_gate = 4 * (f32[4] - want[4]).abs().mean().item()
    steps = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_()
        head.zero_grad()
        kw = {"columns": torch.from_numpy(cols).to(DEV)} if kind == "field" else {"index": y.to(DEV)}
        loss = head.loss(xd, **kw)
        loss.backward()
        steps.append([loss.detach(), xd.grad, head.linear.weight.grad.clone(), head.linear.bias.grad.clone()])
    for name, got, w, t in zip(("loss", "x", "weight", "bias"), steps[0], want, f32):
        err, gate = (got.cpu().double() - w).abs().max().item(), loss_gate if name == "loss" else 4 * (t - w).abs().max().item()
        print("%s n_out=%d %s: error %.3e, gate %.3e" % (kind, n_out, name, err, gate))
        assert err <= gate, name
    assert all(torch.equal(a, b) for a, b in zip(*steps))                         # deterministic=True: two steps, equal bits
    if kind == "field":                                                           # the dense form of the same labels
        same = head.loss(x.to(DEV), labels=ylabel.to(DEV))
        assert abs(same.item() - steps[0][0].item()) <= 2 * loss_gate


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_c_abi_argument_checks():
    lib = _lib.load()
    OK, INVALID, UNSUPPORTED = 0, -1, -2
    f = torch.zeros(64, device=DEV)
    q = torch.zeros(8, dtype=torch.int64, device=DEV)
    i = torch.zeros(16, dtype=torch.int32, device=DEV)
    F, Q, I = f.data_ptr(), q.data_ptr(), i.data_ptr()
    fwd = lambda *a: lib.hgt_class_loss(*a, None)
    bwd = lambda *a: lib.hgt_class_loss_bwd(*a, None)
    assert fwd(None, 0, 0, 0, None, 0, Q, None, 0, None, None, None, None) == OK              # n_rows == 0: nothing is launched
    assert fwd(F, 8, 0, 8, F, 8, None, None, 0, None, F, F, F) == OK
    assert bwd(F, 8, 0, 8, None, 0, None, I, 4, I, F, F, F, F, 8) == OK
    for labels, index, columns in ((None, None, None), (F, Q, None), (F, None, I), (None, Q, I), (F, Q, I)):      # no form, or several
        assert fwd(F, 8, 2, 8, labels, 8, index, columns, 4, None, F, F, F) == INVALID
        assert bwd(F, 8, 2, 8, labels, 8, index, columns, 4, None, F, F, F, F, 8) == INVALID
    for n_rows, n_cols, width in ((-1, 8, 0), (2, -1, 0), (2, 8, -1)):                        # negative sizes
        assert fwd(F, 8, n_rows, n_cols, None, 0, Q, None, width, None, F, F, F) == INVALID
        assert bwd(F, 8, n_rows, n_cols, None, 0, Q, None, width, None, F, F, F, F, 8) == INVALID
    assert fwd(F, 7, 2, 8, None, 0, Q, None, 0, None, F, F, F) == INVALID                     # ld < n_cols
    assert fwd(F, 8, 2, 8, F, 7, None, None, 0, None, F, F, F) == INVALID
    assert bwd(F, 8, 2, 8, None, 0, Q, None, 0, None, F, F, F, F, 7) == INVALID
    assert fwd(F, 8, 2, 8, None, 0, None, I, 0, None, F, F, F) == INVALID                     # width < 1 with columns
    assert bwd(F, 8, 2, 8, None, 0, None, I, 0, None, F, F, F, F, 8) == INVALID
    for outs in ((None, F, F), (F, None, F), (F, F, None)):                                   # NULL outputs
        assert fwd(F, 8, 2, 8, None, 0, Q, None, 0, None, *outs) == INVALID
    for ins in ((None, F, F, F), (F, None, F, F), (F, F, None, F), (F, F, F, None)):
        assert bwd(F, 8, 2, 8, None, 0, Q, None, 0, None, *ins, 8) == INVALID
    assert fwd(F, 2 ** 40, 2, 2 ** 31 - 1024, None, 0, Q, None, 0, None, F, F, F) == UNSUPPORTED
    assert bwd(F, 2 ** 40, 2, 2 ** 31 - 1024, None, 0, Q, None, 0, None, F, F, F, F, 2 ** 40) == UNSUPPORTED
    tr = _lib.HgtSamplerTriple(I, I, I, 0, 1, 0, 0)
    cols = lambda *a: lib.hgt_sampler_label_columns(*a, None)
    assert cols(ctypes.byref(tr), 4, 4, I, 0, I, 8, 0, 0, 0, None, 1, None) == OK
    assert cols(ctypes.byref(tr), 4, 4, I, 2, I, 8, 0, 0, 0, I, 0, I) == INVALID
    assert cols(ctypes.byref(tr), 4, 4, I, 2, I, 8, 0, 0, 0, None, 4, I) == INVALID
    assert cols(ctypes.byref(tr), 4, 4, I, -1, I, 8, 0, 0, 0, I, 4, I) == INVALID
    assert cols(ctypes.byref(tr), 4, 4, I, 2, I, 8, 1, 6, 5, I, 4, I) == INVALID
    assert cols(None, 4, 4, I, 2, I, 8, 0, 0, 0, I, 4, I) == INVALID
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the example
def test_paper_field_example_trains_and_matches_the_torch_chain_at_step_0():
    spec = importlib.util.spec_from_file_location("train_paper_field_device", os.path.join(ROOT, "examples", "train_paper_field_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    small = dict(n_paper=3000, n_hid=32, n_heads=4, n_layers=2, batch_size=64, depth=2, width=32, feat_dim=32, verbose=False, device=DEV,
                 lr=5e-3)
    losses, ndcg = ex.run(steps=24, valid_every=12, **small)                     # thirds of 8 steps: batch noise averages out
    print("losses", " ".join("%.3f" % v for v in losses), " validation NDCG", ndcg)
    assert len(losses) == 24 and np.isfinite(losses).all() and len(ndcg) == 3 and all(0 <= v <= 1 for v in ndcg)
    assert np.mean(losses[-8:]) < np.mean(losses[:8])
    # one step without dropout on the same seeds, by the lists and by torch's chain on the dense labels
    trace = {}
    ours = ex.run(steps=1, dropout=0.0, trace=trace, **small)[0][0]
    theirs = ex.run(steps=1, dropout=0.0, torch_loss=True, **small)[0][0]
    gate = gates(trace["logits"].numpy(), trace["labels"].numpy())[2]
    print("step 0: %.7f against %.7f, gate %.3e" % (ours, theirs, gate.sum() / gate.size))
    assert abs(ours - theirs) <= gate.sum() / gate.size
