"""The task-metric kernels (csrc/hgt_task_metrics.hip) on the GPU against the numpy rule of pyhgt_amd/metrics.py on the same inputs: both
ranks are integers, so the reciprocal rank is bit-equal and NDCG agrees to 1e-12 (fp64 sums of at most P terms, test_task_metrics.py);
the loss kernels against float64 autograd of the formula, gated by the fp32 error of torch.log_softmax on the CPU on the same inputs
(also at every multiple of the block of 256, for one segment and for 100 000, through strided and offset views, and with inf / NaN scores);
and three steps of examples/train_author_disambiguation_device.py.  Reads committed fixtures only."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from pyhgt_amd import _lib, metrics as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CAP = _lib.RANK_LIST_CAP
NDCG_TOL = 1e-12


def _agree(scores, labels=None, index=None, k=None, sizes=None):
    """the device call against the rule on host copies of the same arrays -> (ndcg, rr) as numpy"""
    host = lambda t: None if t is None else t.cpu().numpy()
    ndcg, rr = M.rank_metrics(scores, labels=labels, index=index, k=k, sizes=sizes)
    assert ndcg.dtype == rr.dtype == torch.float64 and ndcg.device == rr.device == scores.device
    want_ndcg, want_rr = M.np_rank_metrics(host(scores), host(labels), host(index), k, sizes)
    ndcg, rr = ndcg.cpu().numpy(), rr.cpu().numpy()
    assert ndcg.shape == rr.shape == want_rr.shape
    assert np.array_equal(rr, want_rr, equal_nan=True)                                    # integer ranks: bit-equal
    assert np.array_equal(np.isnan(ndcg), np.isnan(want_ndcg))
    if ndcg.size:
        assert np.nanmax(np.abs(ndcg - want_ndcg), initial=0.0) <= NDCG_TOL
    return ndcg, rr


def _dense(rng, n, c, p_mean=7.0, graded=True):
    l = (rng.random((n, c)) < min(1.0, p_mean / max(c, 1))).astype(np.float32)
    if graded:
        l *= rng.integers(1, 5, size=(n, c)).astype(np.float32) / 4
    return l


@pytest.mark.parametrize("c", [1, 3, 63, 64, 65, 255, 256, 257, 4099])
def test_regular_rows_all_three_relevance_forms(c):
    rng = np.random.default_rng(c)
    for n in (0, 1, 3, 300):
        s = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32)).to(DEV)
        tied = torch.from_numpy(rng.integers(0, 6, size=(n, c)).astype(np.float32)).to(DEV)      # many equal scores
        labels = torch.from_numpy(_dense(rng, n, c)).to(DEV)
        index = torch.from_numpy(rng.integers(-1, c, size=n)).to(DEV)
        for scores in (s, tied):
            _agree(scores, labels=labels)
            _agree(scores, index=index)
            _agree(scores)
        _agree(tied, labels=labels, k=1)
        _agree(s, labels=labels, k=max(1, c // 3))
        _agree(s, index=index, k=c + 5)


@pytest.mark.parametrize("c", [3, 64, 65, 256, 4099])
def test_column_slice_of_a_wider_tensor(c):
    """row stride c + 1 and a base 4 bytes off: the rows are read in place, 16-byte loads only where a row's base allows"""
    rng = np.random.default_rng(100 + c)
    n = 9
    wide_s = torch.from_numpy(rng.integers(0, 50, size=(n, c + 1)).astype(np.float32)).to(DEV)
    wide_l = torch.from_numpy(_dense(rng, n, c + 1)).to(DEV)
    s, l = wide_s[:, 1:], wide_l[:, 1:]
    assert s.stride(0) == c + 1 and s.data_ptr() % 16 == 4
    a = _agree(s, labels=l)
    b = _agree(s.contiguous(), labels=l.contiguous())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _agree(s, index=torch.arange(n, device=DEV) % c)
    _agree(s, labels=l.contiguous(), k=2)                                                 # two different strides in one call


def test_number_of_positives_on_both_sides_of_every_list_line():
    """P = 0, 1, 7, the line between the two counting schemes (16 | 17), every line at which a thread of the second scheme takes one
    more list entry or the tile is shared between fewer groups (64, 128, 192, 256, 384, 512, 768 and the next), the list capacity - 1,
    exactly and + 1 (the first row that needs a second pass), several passes, and P = C"""
    c = 4099
    counts = [0, 1, 7, 16, 17, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 513, 768, 769, CAP - 1, CAP, CAP + 1, 2 * CAP,
              2 * CAP + 1, 3 * CAP + 500, c]
    rng = np.random.default_rng(5)
    l = np.zeros((len(counts), c), np.float32)
    for r, p in enumerate(counts):
        l[r, rng.choice(c, size=p, replace=False)] = rng.integers(1, 9, size=p).astype(np.float32) / 8
    labels = torch.from_numpy(l).to(DEV)
    for s in (rng.standard_normal((len(counts), c)), rng.integers(0, 40, size=(len(counts), c))):
        scores = torch.from_numpy(s.astype(np.float32)).to(DEV)
        _agree(scores, labels=labels)
        _agree(scores, labels=labels, k=100)
    # the positives packed at the end of the row, and at its start: the walk that fills the list stops and resumes inside a tile
    for lo in (0, c - (CAP + 1)):
        l = np.zeros((1, c), np.float32)
        l[0, lo:lo + CAP + 1] = 1.0
        _agree(scores[:1], labels=torch.from_numpy(l).to(DEV))
    for cc in (1, 5, 64, 65, 300):                                                        # P = C on both kernels
        s = torch.from_numpy(rng.integers(0, 9, size=(4, cc)).astype(np.float32)).to(DEV)
        _agree(s, labels=torch.ones(4, cc, device=DEV))
        _agree(s, labels=torch.from_numpy(rng.integers(1, 4, size=(4, cc)).astype(np.float32)).to(DEV), k=3)


def test_ties_and_special_scores():
    for c in (66, 130, 300):                                                              # equal scores at positions 63 and 64
        s = np.arange(c, dtype=np.float32)[None].repeat(4, 0)
        s[:, 63] = s[:, 64] = 1000.0
        ndcg, rr = _agree(torch.from_numpy(s).to(DEV), index=torch.tensor([63, 64, 0, c - 1], device=DEV))
        assert rr.tolist() == [1.0, 0.5, 1.0 / c, 1.0 / 3]
    for c in (2, 64, 65, 300, 1100):                                                      # a whole row of equal scores
        s = torch.full((3, c), 2.5, device=DEV)
        ndcg, rr = _agree(s, index=torch.tensor([0, c // 2, c - 1], device=DEV))
        assert rr.tolist() == [1.0, 1.0 / (c // 2 + 1), 1.0 / c]
        _agree(s, labels=torch.ones(3, c, device=DEV))
    rng = np.random.default_rng(9)
    for c in (20, 64, 300):                                                               # -inf is an ordinary score
        s = rng.standard_normal((5, c)).astype(np.float32)
        s[rng.random((5, c)) < 0.3] = -np.inf
        s[0] = -np.inf
        _agree(torch.from_numpy(s).to(DEV), index=torch.from_numpy(rng.integers(0, c, size=5)).to(DEV))
        _agree(torch.from_numpy(s).to(DEV), labels=torch.from_numpy(_dense(rng, 5, c, 5.0)).to(DEV))
    for c in (20, 64, 65, 300, 2100):                                                     # one NaN row among clean ones
        s = rng.standard_normal((6, c)).astype(np.float32)
        s[2, c - 1] = np.nan
        for kw in (dict(), dict(index=torch.full((6,), -1, dtype=torch.int64, device=DEV)),
                   dict(labels=torch.from_numpy(_dense(rng, 6, c, 3.0)).to(DEV))):
            ndcg, rr = _agree(torch.from_numpy(s).to(DEV), **kw)
            assert np.isnan(ndcg).tolist() == np.isnan(rr).tolist() == [False, False, True, False, False, False]
    ndcg, rr = _agree(torch.zeros(4, 0, device=DEV))                                      # C = 0
    assert ndcg.tolist() == rr.tolist() == [0.0] * 4


def test_ragged_rows_on_both_sides_of_the_wavefront_line():
    rng = np.random.default_rng(11)
    sizes = np.array([1, 2, 4, 63, 64, 65, 1000, 0, 64, 1, 65, 4, 1000, 2, 63, 6, 6, 6])
    total = int(sizes.sum())
    for s in (rng.standard_normal(total), rng.integers(0, 5, size=total)):
        scores = torch.from_numpy(s.astype(np.float32)).to(DEV)
        ndcg, rr = _agree(scores, sizes=sizes)                                            # the first of every segment is the positive
        assert ndcg[7] == rr[7] == 0.0 and ndcg[0] == rr[0] == 1.0
        seg = M.Segments(sizes, DEV)
        a, b = M.rank_metrics(scores, sizes=seg)
        assert np.array_equal(a.cpu().numpy(), ndcg) and np.array_equal(b.cpu().numpy(), rr)
        _agree(scores, sizes=sizes, k=3)
        index = torch.from_numpy(np.array([rng.integers(-1, max(c, 1)) for c in sizes])).to(DEV)
        _agree(scores, index=index, sizes=sizes)
        labels = torch.from_numpy((rng.random(total) < 0.3).astype(np.float32) * rng.integers(1, 4, size=total).astype(np.float32)).to(DEV)
        _agree(scores, labels=labels, sizes=sizes)
    small = np.array([4, 6, 5, 4, 64, 7])                                                 # nothing longer than a wavefront: one launch
    _agree(torch.from_numpy(rng.standard_normal(int(small.sum())).astype(np.float32)).to(DEV), sizes=small)
    ndcg, rr = M.rank_metrics(torch.zeros(0, device=DEV), sizes=[])                       # an empty segment list
    assert ndcg.shape == rr.shape == (0,) and ndcg.dtype == torch.float64 and ndcg.is_cuda
    with pytest.raises(TypeError):
        M.rank_metrics(torch.zeros(3, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        M.rank_metrics(torch.zeros(5, device=DEV), sizes=[2, 2])


def test_a_row_does_not_depend_on_the_call_around_it():
    rng = np.random.default_rng(13)
    for c in (40, 257, 2500):
        n = 50
        scores = torch.from_numpy(rng.integers(0, 30, size=(n, c)).astype(np.float32)).to(DEV)
        labels = torch.from_numpy(_dense(rng, n, c, 12.0)).to(DEV)
        labels[7] = 1.0                                                                   # a row of several passes at c = 2500
        ndcg, rr = M.rank_metrics(scores, labels=labels)
        again = M.rank_metrics(scores, labels=labels)
        assert torch.equal(ndcg, again[0]) and torch.equal(rr, again[1])
        for r in (0, 7, 49):
            one = M.rank_metrics(scores[r:r + 1], labels=labels[r:r + 1])
            assert torch.equal(one[0], ndcg[r:r + 1]) and torch.equal(one[1], rr[r:r + 1])
    sizes = [5, 1000, 64, 65, 7]
    flat = torch.from_numpy(rng.standard_normal(sum(sizes)).astype(np.float32)).to(DEV)
    ndcg, rr = M.rank_metrics(flat, sizes=sizes)
    one = M.rank_metrics(flat[5:1005].reshape(1, 1000), index=torch.zeros(1, dtype=torch.int64, device=DEV))
    assert torch.equal(one[0], ndcg[1:2]) and torch.equal(one[1], rr[1:2])


# ---------------------------------------------------------------------------------------------------------------- the loss
LOSS_SIZES = [2, 3, 63, 64, 65, 1000, 2, 64, 65, 3, 1000, 4, 10, 6]


def _terms(x, sizes):
    """the formula per segment with torch on the CPU in x's dtype: -log_softmax(seg)[0] / ln(l)"""
    out, beg = [], 0
    for l in sizes:
        out.append(-torch.log_softmax(x[beg:beg + l], dim=-1)[0] / math.log(l))
        beg += l
    return torch.stack(out)


@pytest.fixture(scope="module")
def loss_case():
    """scores in +-30, one segment with a dominant entry of 80; float64 terms and gradient, and the fp32 torch yardstick of both"""
    rng = np.random.default_rng(17)
    x = rng.uniform(-30, 30, size=sum(LOSS_SIZES)).astype(np.float32)
    x[sum(LOSS_SIZES[:5]) + 123] = 80.0                                                   # inside the first segment of 1000
    wts = rng.uniform(0.5, 2.0, size=len(LOSS_SIZES)).astype(np.float32)
    case = {"x": x, "wts": wts}
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        t = torch.from_numpy(x).to(dtype).requires_grad_()
        terms = _terms(t, LOSS_SIZES)
        (terms * torch.from_numpy(wts).to(dtype)).sum().backward()
        case["terms" + tag], case["grad" + tag] = terms.detach().double().numpy(), t.grad.double().numpy()
    return case


def test_pair_rank_loss_forward_and_gradient_against_float64(loss_case):
    """Gate: the error of torch.log_softmax in fp32 on the CPU on the same inputs against the same float64 values, times 4 (a
    different but equally legitimate summation order).  Per segment the yardstick is the largest fp32 error of a segment's term, per
    gradient element the largest fp32 error of an element.  The sum of the n terms is gated by 4 x the sum of the per-segment fp32
    errors plus the rounding of an fp32 sum of n values, (n - 1) * 2^-24 * sum |term|."""
    x, wts = loss_case["x"], loss_case["wts"]
    t64, g64 = loss_case["terms64"], loss_case["grad64"]
    yard_terms, yard_grad = np.abs(loss_case["terms32"] - t64), np.abs(loss_case["grad32"] - g64)
    scores = torch.from_numpy(x).to(DEV).requires_grad_()
    terms = M.pair_rank_loss(scores, LOSS_SIZES, reduce=False)
    assert terms.dtype == torch.float32 and terms.shape == (len(LOSS_SIZES),)
    (terms * torch.from_numpy(wts).to(DEV)).sum().backward()
    err_terms = np.abs(terms.detach().cpu().double().numpy() - t64)
    err_grad = np.abs(scores.grad.cpu().double().numpy() - g64)
    total = M.pair_rank_loss(scores.detach(), M.Segments(LOSS_SIZES, DEV))
    err_total = abs(float(total.item()) - t64.sum())
    gate_total = 4 * yard_terms.sum() + (len(LOSS_SIZES) - 1) * 2.0 ** -24 * np.abs(t64).sum()
    print("loss terms: kernel max err %.3e, torch fp32 max err %.3e; gradient: kernel %.3e, torch fp32 %.3e; total: kernel %.3e, gate %.3e"
          % (err_terms.max(), yard_terms.max(), err_grad.max(), yard_grad.max(), err_total, gate_total))
    assert abs(t64.sum() - M.np_pair_rank_loss(x, LOSS_SIZES)) < 1e-10                    # the float64 reference is the rule
    assert err_terms.max() <= 4 * yard_terms.max()
    assert err_grad.max() <= 4 * yard_grad.max()
    assert err_total <= gate_total
    # the same bits every time, and through the sum
    again = M.pair_rank_loss(scores.detach().requires_grad_(), LOSS_SIZES, reduce=False)
    assert torch.equal(again.detach(), terms.detach())
    s2 = torch.from_numpy(x).to(DEV).requires_grad_()
    M.pair_rank_loss(s2, LOSS_SIZES).backward()
    ones = torch.from_numpy(x).double().requires_grad_()
    _terms(ones, LOSS_SIZES).sum().backward()
    ones32 = torch.from_numpy(x).requires_grad_()
    _terms(ones32, LOSS_SIZES).sum().backward()
    assert np.abs(s2.grad.cpu().double().numpy() - ones.grad.numpy()).max() <= 4 * (ones32.grad.double() - ones.grad).abs().max().item()


def test_loss_backward_writes_every_element_once_and_argument_errors(loss_case):
    lib = _lib.load()
    x = torch.from_numpy(loss_case["x"]).to(DEV)
    seg = M.Segments(LOSS_SIZES, DEV)
    st = torch.cuda.current_stream().cuda_stream
    loss = torch.full((seg.n,), float("nan"), device=DEV)
    lse = torch.full((seg.n, 2), float("nan"), device=DEV)
    assert lib.hgt_segment_first_nll(x.data_ptr(), seg.row_ptr.data_ptr(), seg.n, seg.longest, loss.data_ptr(), lse.data_ptr(), st) == 0
    assert not torch.isnan(loss).any() and not torch.isnan(lse).any()
    m = torch.stack([x[b:b + l].max() for b, l in zip(np.cumsum([0] + LOSS_SIZES[:-1]).tolist(), LOSS_SIZES)])
    assert torch.equal(lse[:, 0], m)
    grads = []
    for poison in (float("nan"), 7.0):                                                    # a poisoned output: nothing of it survives
        grad = torch.full((seg.total + 8,), poison, device=DEV)
        g = torch.ones(seg.n, device=DEV)
        assert lib.hgt_segment_first_nll_bwd(x.data_ptr(), seg.row_ptr.data_ptr(), seg.n, seg.longest, lse.data_ptr(), g.data_ptr(),
                                             grad.data_ptr(), st) == 0
        assert not torch.isnan(grad[:seg.total]).any()
        tail = grad[seg.total:]
        assert torch.isnan(tail).all() if poison != poison else (tail == poison).all()    # and nothing past the end is touched
        grads.append(grad[:seg.total].clone())
    assert torch.equal(grads[0], grads[1])
    with pytest.raises(ValueError):
        M.pair_rank_loss(x[:5], [4, 1])
    with pytest.raises(ValueError):
        M.pair_rank_loss(x[:5], [2, 2])
    with pytest.raises(TypeError):
        M.pair_rank_loss(x[:4].double(), [2, 2])
    empty = M.pair_rank_loss(torch.zeros(0, device=DEV), [])
    assert empty.item() == 0.0


# ---------------------------------------------------------------------------------------------------------------- the loss at its line edges
EDGE_SIZES = [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 5000]                       # both sides of every multiple of the block of 256
EQUAL_SIZES = [2, 64, 65, 256, 1000]                                                      # segments of equal scores: the term is 1


def _both(x, sizes, wts, terms_fn=_terms):
    """float64 terms and gradient of sum(wts * terms), and the same in torch float32 on the CPU: the truth and the yardstick"""
    out = []
    for dtype in (torch.float64, torch.float32):
        t = torch.from_numpy(x).to(dtype).requires_grad_()
        terms = terms_fn(t, sizes)
        (terms * torch.from_numpy(wts).to(dtype)).sum().backward()
        out += [terms.detach().double().numpy(), t.grad.double().numpy()]
    return out


def _device(x, sizes, wts):
    scores = torch.from_numpy(x).to(DEV).requires_grad_()
    terms = M.pair_rank_loss(scores, sizes, reduce=False)
    (terms * torch.from_numpy(wts).to(DEV)).sum().backward()
    return terms.detach().cpu().double().numpy(), scores.grad.cpu().double().numpy()


def test_loss_on_both_sides_of_every_block_multiple_with_the_true_entry_at_either_end():
    """Segments of 255 .. 1025 and 5000 scores: a thread of the workgroup kernel walks 1 .. 20 entries, some threads one fewer.  The
    true (first) entry is the row maximum in every third segment and the row minimum in every third; five segments hold equal scores,
    where the term is ln(l) / ln(l) = 1.  Gate: 4 x the largest float32 error of torch over the segments of the case."""
    rng = np.random.default_rng(23)
    sizes = EDGE_SIZES + EQUAL_SIZES
    x = rng.uniform(-30, 30, size=sum(sizes)).astype(np.float32)
    beg = np.concatenate([[0], np.cumsum(sizes)])
    for i in range(len(EDGE_SIZES)):
        if i % 3 == 0:
            x[beg[i]] = 31.0
        elif i % 3 == 1:
            x[beg[i]] = -31.0
    for i, v in zip(range(len(EDGE_SIZES), len(sizes)), (2.5, -30.0, 0.0, 1e4, -7.25)):
        x[beg[i]:beg[i + 1]] = v
    wts = rng.uniform(0.5, 2.0, size=len(sizes)).astype(np.float32)
    t64, g64, t32, g32 = _both(x, sizes, wts)
    terms, grad = _device(x, sizes, wts)
    gate_t, gate_g = 4 * np.abs(t32 - t64).max(), 4 * np.abs(g32 - g64).max()
    print("loss at the block lines: terms max err %.3e (gate %.3e), gradient %.3e (gate %.3e); equal scores: |term - 1| max %.3e"
          % (np.abs(terms - t64).max(), gate_t, np.abs(grad - g64).max(), gate_g, np.abs(terms[len(EDGE_SIZES):] - 1).max()))
    assert abs(t64.sum() - M.np_pair_rank_loss(x, sizes)) < 1e-9
    assert np.abs(t64[len(EDGE_SIZES):] - 1).max() < 1e-12
    assert np.abs(terms - t64).max() <= gate_t and np.abs(grad - g64).max() <= gate_g
    assert np.abs(terms[len(EDGE_SIZES):] - 1).max() <= gate_t


def test_loss_of_a_single_segment_on_either_kernel():
    """n_seg = 1: one wavefront of a workgroup of four has a segment (lengths <= 64), or the grid is one workgroup (longer).  The case
    is the family of these calls: each is gated by 4 x the largest float32 error of torch over the family."""
    rng = np.random.default_rng(29)
    lengths = [2, 5, 33, 64, 65, 300, 1024, 5000]
    runs = []
    for l in lengths:
        x = rng.uniform(-30, 30, size=l).astype(np.float32)
        wts = np.array([1.5], np.float32)
        runs.append(_both(x, [l], wts) + list(_device(x, [l], wts)))
    gate_t = 4 * max(np.abs(r[2] - r[0]).max() for r in runs)
    gate_g = 4 * max(np.abs(r[3] - r[1]).max() for r in runs)
    for l, (t64, g64, t32, g32, terms, grad) in zip(lengths, runs):
        print("one segment of %d: term err %.3e (gate %.3e), gradient err %.3e (gate %.3e)" % (l, abs(terms[0] - t64[0]), gate_t,
                                                                                                np.abs(grad - g64).max(), gate_g))
        assert terms.shape == (1,) and abs(terms[0] - t64[0]) <= gate_t and np.abs(grad - g64).max() <= gate_g


def test_loss_of_a_hundred_thousand_pairs():
    """100 000 segments of two scores: 25 000 workgroups of the wavefront kernel, two live lanes each"""
    n = 100000
    rng = np.random.default_rng(31)
    x = rng.uniform(-30, 30, size=2 * n).astype(np.float32)
    wts = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
    pairs = lambda t, sizes: -torch.log_softmax(t.view(-1, 2), dim=1)[:, 0] / math.log(2)     # _terms for equal lengths, in one call
    t64, g64, t32, g32 = _both(x, None, wts, terms_fn=pairs)
    probe = rng.choice(n, size=50, replace=False)
    for r in probe:                                                                       # the one call is the formula of _terms
        assert abs(_terms(torch.from_numpy(x[2 * r:2 * r + 2]).double(), [2])[0].item() - t64[r]) < 1e-12
    terms, grad = _device(x, np.full(n, 2), wts)
    print("100000 pairs: terms max err %.3e (torch float32 %.3e), gradient %.3e (torch float32 %.3e)"
          % (np.abs(terms - t64).max(), np.abs(t32 - t64).max(), np.abs(grad - g64).max(), np.abs(g32 - g64).max()))
    assert np.abs(terms - t64).max() <= 4 * np.abs(t32 - t64).max() and np.abs(grad - g64).max() <= 4 * np.abs(g32 - g64).max()
    total = M.pair_rank_loss(torch.from_numpy(x).to(DEV), np.full(n, 2))
    unit = _both(x, None, np.ones(n, np.float32), terms_fn=pairs)
    assert abs(total.item() - unit[0].sum()) <= 4 * np.abs(unit[2] - unit[0]).sum() + (n - 1) * 2.0 ** -24 * np.abs(unit[0]).sum()


@pytest.mark.parametrize("view", ["every_second", "offset"])
def test_loss_gradient_reaches_a_strided_or_offset_view_and_nothing_else(view):
    """scores = wide[1::2], or a slice that starts 5 elements into its storage: the gradient arrives at those elements of `wide`; every
    other element gets its gradient from a second leaf alone, a sentinel that must come through bit for bit"""
    sizes = [3, 64, 65, 300, 2]
    L = sum(sizes)
    rng = np.random.default_rng(37)
    x = rng.uniform(-30, 30, size=L).astype(np.float32)
    wts = rng.uniform(0.5, 2.0, size=len(sizes)).astype(np.float32)
    t64, g64, t32, g32 = _both(x, sizes, wts)
    if view == "every_second":
        host, mine = np.full(2 * L, 99.0, np.float32), np.zeros(2 * L, bool)
        mine[1::2] = True
        pick = lambda w: w[1::2]
    else:
        host, mine = np.full(L + 12, 99.0, np.float32), np.zeros(L + 12, bool)
        mine[5:5 + L] = True
        pick = lambda w: w[5:][:L]
    host[mine] = x
    wide = torch.from_numpy(host).to(DEV).requires_grad_()
    sentinel = torch.full((int((~mine).sum()),), -12345.5, device=DEV, requires_grad=True)
    scores = pick(wide)
    assert scores.data_ptr() != wide.data_ptr() and (scores.stride(0) == 2 or scores.storage_offset() == 5)
    terms = M.pair_rank_loss(scores, sizes, reduce=False)
    ((terms * torch.from_numpy(wts).to(DEV)).sum() + (wide[torch.from_numpy(~mine).to(DEV)] * sentinel).sum()).backward()
    grad = wide.grad.cpu().numpy()
    assert np.array_equal(grad[~mine], np.full(int((~mine).sum()), -12345.5, np.float32))
    assert torch.equal(sentinel.grad, torch.full_like(sentinel, 99.0))
    assert np.abs(terms.detach().cpu().double().numpy() - t64).max() <= 4 * np.abs(t32 - t64).max()
    assert np.abs(grad[mine].astype(np.float64) - g64).max() <= 4 * np.abs(g32 - g64).max()
    plain = _device(x, sizes, wts)                                                        # the same bits as from a contiguous vector
    assert np.array_equal(plain[0], terms.detach().cpu().double().numpy()) and np.array_equal(plain[1], grad[mine].astype(np.float64))


NONFINITE = [("minus_inf_inside", lambda seg: seg.__setitem__(len(seg) // 2, -np.inf)),
             ("minus_inf_first", lambda seg: seg.__setitem__(0, -np.inf)),
             ("all_minus_inf", lambda seg: seg.__setitem__(slice(None), -np.inf)),
             ("plus_inf", lambda seg: seg.__setitem__(len(seg) - 1, np.inf)),
             ("one_nan", lambda seg: seg.__setitem__(1, np.nan))]


@pytest.mark.parametrize("length", [40, 64, 65, 300])
def test_loss_with_non_finite_scores_agrees_with_torch_log_softmax(length):
    """-inf inside a segment (an ordinary score: weight 0), -inf first (the term is +inf, the gradient finite), a whole segment of
    -inf, +inf and one NaN (torch gives NaN throughout such a segment), each between two clean segments, in a segment a wavefront
    takes and in one a workgroup takes.  Against torch.log_softmax in float32 on the CPU: inf and NaN sit at the same positions of the
    terms and of the gradient, with the same sign; the finite entries are within 4 x torch's float32 error over the finite entries of
    the case; and the clean segments come out bit for bit as from a call without the others."""
    rng = np.random.default_rng(41 + length)
    sizes = [length if i % 2 else (7, 70)[(i // 2) % 2] for i in range(2 * len(NONFINITE) + 1)]      # clean, special, clean, ...
    beg = np.concatenate([[0], np.cumsum(sizes)])
    x = rng.uniform(-20, 20, size=sum(sizes)).astype(np.float32)
    for i, (_, put) in enumerate(NONFINITE):
        put(x[beg[2 * i + 1]:beg[2 * i + 2]])
    wts = rng.uniform(0.5, 2.0, size=len(sizes)).astype(np.float32)
    t64, g64, t32, g32 = _both(x, sizes, wts)
    terms, grad = _device(x, sizes, wts)
    want_terms = {"minus_inf_inside": np.isfinite, "minus_inf_first": np.isposinf, "all_minus_inf": np.isnan, "plus_inf": np.isnan,
                  "one_nan": np.isnan}
    for i, (name, _) in enumerate(NONFINITE):                                             # what torch gives is what the docstring says
        assert want_terms[name](t32[2 * i + 1]), name
        seg = g32[beg[2 * i + 1]:beg[2 * i + 2]]
        assert np.isfinite(seg).all() if name.startswith("minus_inf") else np.isnan(seg).all(), name
    for got, f32, f64, what in ((terms, t32, t64, "terms"), (grad, g32, g64, "gradient")):
        assert np.array_equal(np.isnan(got), np.isnan(f32)), what
        assert np.array_equal(np.isposinf(got), np.isposinf(f32)) and np.array_equal(np.isneginf(got), np.isneginf(f32)), what
        fin = np.isfinite(f32)
        assert np.array_equal(np.isfinite(f64), fin)
        err, yard = np.abs(got[fin] - f64[fin]).max(), np.abs(f32[fin] - f64[fin]).max()
        print("non-finite scores, length %d: %s: %d finite entries, max err %.3e, torch float32 %.3e" % (length, what, fin.sum(), err, yard))
        assert err <= 4 * yard, what
    clean = np.arange(0, len(sizes), 2)
    keep = np.concatenate([np.arange(beg[i], beg[i + 1]) for i in clean])
    alone = _device(x[keep], [sizes[i] for i in clean], wts[clean])
    assert np.array_equal(alone[0], terms[clean]) and np.array_equal(alone[1], grad[keep])


def test_author_disambiguation_example_runs_three_steps():
    spec = importlib.util.spec_from_file_location("train_author_disambiguation_device",
                                                  os.path.join(ROOT, "examples", "train_author_disambiguation_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    losses, valid, sizes = ex.run(steps=3, n_paper=400, n_hid=32, n_heads=4, n_layers=2, batch_size=32, depth=2, width=16, feat_dim=32,
                                  valid_every=1, verbose=False, device=DEV)
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    assert len(valid) == 3 and all(0.0 <= v <= 1.0 for pair in valid for v in pair)
    assert sizes.size > 0 and sizes.min() >= 4
