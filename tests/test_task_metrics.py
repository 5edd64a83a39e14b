"""CPU tests of the task metrics (pyhgt_amd/metrics.py): the numpy rule against the recorded results of the reference's own
`ndcg_at_k` / `mean_reciprocal_rank` (tests/golden/task/metrics_small.npz, written by tools/gen_golden_metrics.py), live against the
reference where its tree is present, hand-written expectations for ties, -inf, NaN and the empty cases, the float64 loss, and the
boundary: header, bindings and Makefile list the new file and symbols and the ABI is still 8."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from pyhgt_amd import _lib, metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "task", "metrics_small.npz")
NEW_SYMBOLS = ("hgt_rank_metrics", "hgt_segment_first_nll", "hgt_segment_first_nll_bwd")
# DCG and IDCG are float64 sums of at most P terms with a log2 good to 2 ulp: (P + 8) * 2^-52 relative each, under 1e-12 for P <= 4096
NDCG_TOL = 1e-12


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _per_k(scores, labels, sizes, ks):
    """np_rank_metrics row by row (k differs between the rows of the fixture)"""
    ndcg, rr, beg = [], [], 0
    for c, k in zip(sizes.tolist(), ks.tolist()):
        a, b = M.np_rank_metrics(scores[beg:beg + c][None], labels=labels[beg:beg + c][None], k=k or None)
        ndcg.append(a[0]), rr.append(b[0])
        beg += c
    return np.asarray(ndcg), np.asarray(rr)


def test_rule_equals_the_recorded_reference_results(golden):
    scores, labels, sizes, ks = (golden["rank/" + n] for n in ("scores", "labels", "sizes", "k"))
    beg = 0
    for c in sizes.tolist():                                          # every case has distinct scores and at most 4096 positives
        assert np.unique(scores[beg:beg + c]).size == c and (labels[beg:beg + c] > 0).sum() <= 4096
        beg += c
    assert sizes.size >= 30 and sizes.max() >= 3000
    ndcg, rr = _per_k(scores, labels, sizes, ks)
    assert np.array_equal(rr, golden["rank/mrr"])
    assert np.abs(ndcg - golden["rank/ndcg"]).max() <= NDCG_TOL
    # k = None rows in one ragged call give the same numbers
    sel = np.flatnonzero(ks == 0)
    off = np.concatenate([[0], np.cumsum(sizes)])
    cat = lambda a: np.concatenate([a[off[i]:off[i + 1]] for i in sel])
    n2, r2 = M.np_rank_metrics(cat(scores), labels=cat(labels), sizes=sizes[sel])
    assert np.array_equal(n2, ndcg[sel]) and np.array_equal(r2, rr[sel])


def test_rule_equals_the_live_reference_on_fresh_rows():
    from oracle.reference_loader import reference_available, load_reference_data
    if not reference_available():
        pytest.skip("reference tree not present")
    G = _tool("gen_golden_metrics")
    data = load_reference_data()
    scores, labels, sizes, ks = G.make_rows(seed=12345)
    want_ndcg, want_mrr = G.reference_rows(data, scores, labels, sizes, ks)
    ndcg, rr = _per_k(scores, labels, sizes, ks)
    assert np.array_equal(rr, want_mrr)
    assert np.abs(ndcg - want_ndcg).max() <= NDCG_TOL


def w(i):
    return 1.0 if i == 0 else 1.0 / math.log2(i + 1)


def test_ties_go_to_the_lower_position():
    s = np.float32([[2, 5, 5, 1, 5]])
    assert M.np_ranks(s[0]).tolist() == [3, 0, 1, 4, 2]
    for idx, rank in ((1, 0), (2, 1), (4, 2), (0, 3), (3, 4)):
        ndcg, rr = M.np_rank_metrics(s, index=[idx])
        assert rr[0] == 1.0 / (1 + rank) and abs(ndcg[0] - w(rank)) < 1e-15
    ndcg, rr = M.np_rank_metrics(np.zeros((1, 70), np.float32), index=[64])              # a whole row of equal scores
    assert rr[0] == 1.0 / 65 and abs(ndcg[0] - w(64)) < 1e-15
    ndcg, rr = M.np_rank_metrics(np.float32([[0.0, -0.0]]), index=[1])                    # -0.0 == 0.0
    assert rr[0] == 0.5


def test_ideal_ranks_of_graded_relevances():
    s = np.float32([[4, 3, 2, 1]])
    l = np.float32([[0, 1, 2, 2]])                                                        # ideal order: positions 2, 3, 1
    ndcg, rr = M.np_rank_metrics(s, labels=l)
    dcg = 1 * w(1) + 2 * w(2) + 2 * w(3)
    idcg = 2 * w(0) + 2 * w(1) + 1 * w(2)
    assert abs(ndcg[0] - dcg / idcg) < 1e-15 and rr[0] == 0.5
    ndcg, rr = M.np_rank_metrics(s, labels=l, k=2)                                        # k < C: rr does not depend on k
    assert abs(ndcg[0] - (1 * w(1)) / (2 * w(0) + 2 * w(1))) < 1e-15 and rr[0] == 0.5
    n9, r9 = M.np_rank_metrics(s, labels=l, k=9)                                          # k > C is k = C
    n0, r0 = M.np_rank_metrics(s, labels=l)
    assert n9[0] == n0[0] and r9[0] == r0[0]


def test_special_scores_and_empty_cases():
    inf = np.inf
    ndcg, rr = M.np_rank_metrics(np.float32([[-inf, 1, -inf, 0]]), index=[2])            # -inf is an ordinary score; it ties with itself
    assert rr[0] == 0.25 and abs(ndcg[0] - w(3)) < 1e-15
    ndcg, rr = M.np_rank_metrics(np.float32([[-inf, 1, -inf, 0]]), index=[0])
    assert rr[0] == 1.0 / 3
    s = np.float32([[1, 2, 3], [1, np.nan, 3], [3, 2, 1]])
    ndcg, rr = M.np_rank_metrics(s, index=[0, 0, 0])                                      # only the NaN row is NaN
    assert np.isnan(ndcg).tolist() == [False, True, False] and np.isnan(rr).tolist() == [False, True, False]
    assert rr[0] == 1.0 / 3 and rr[2] == 1.0
    ndcg, rr = M.np_rank_metrics(s[[0, 2]], index=[-1, 7])                                # index = -1 (or past the row): P = 0
    assert ndcg.tolist() == [0, 0] and rr.tolist() == [0, 0]
    ndcg, rr = M.np_rank_metrics(s[[0]], labels=np.zeros((1, 3), np.float32))             # P = 0, dense
    assert ndcg.tolist() == [0] and rr.tolist() == [0]
    ndcg, rr = M.np_rank_metrics(np.zeros((2, 0), np.float32))                            # C = 0
    assert ndcg.tolist() == [0, 0] and rr.tolist() == [0, 0]
    ndcg, rr = M.np_rank_metrics(np.zeros((0, 5), np.float32))
    assert ndcg.shape == rr.shape == (0,)
    ndcg, rr = M.np_rank_metrics(np.float32([3, 1, 2, 5, 4]), sizes=[3, 0, 2])            # first form on ragged rows, one of them empty
    assert rr.tolist() == [1.0, 0.0, 1.0] and ndcg.tolist() == [1.0, 0.0, 1.0]
    ndcg, rr = M.np_rank_metrics(np.float32([1, 3, 2, 4, 5]), sizes=[3, 2])
    assert rr.tolist() == [1.0 / 3, 0.5]


def test_argument_errors_and_the_cpu_tensor_path():
    s = torch.tensor([[0.5, 2.0, 1.0], [3.0, 2.0, 1.0]])
    ndcg, rr = M.rank_metrics(s, index=torch.tensor([0, 0]))
    assert ndcg.dtype == rr.dtype == torch.float64 and rr.tolist() == [1.0 / 3, 1.0]
    ndcg, rr = M.rank_metrics(s.reshape(-1), sizes=[2, 4], k=1)
    assert rr.tolist() == [0.5, 1.0 / 3] and ndcg.tolist() == [0.0, 0.0]
    with pytest.raises(TypeError):
        M.rank_metrics(s.double())
    with pytest.raises(TypeError):
        M.rank_metrics(s.half())
    with pytest.raises(ValueError):
        M.rank_metrics(s, labels=torch.zeros(2, 3), index=torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError):
        M.rank_metrics(s, k=0)
    with pytest.raises(ValueError):
        M.rank_metrics(s.reshape(-1), sizes=[2, 3])
    with pytest.raises(ValueError):
        M.np_pair_rank_loss(np.zeros(5, np.float32), [4, 1])                              # the reference divides by log 1 = 0 there
    with pytest.raises(ValueError):
        M.np_pair_rank_loss(np.zeros(5, np.float32), [2, 2])
    with pytest.raises(RuntimeError):
        M.pair_rank_loss(torch.zeros(4), [2, 2])                                          # no CPU fallback of the loss kernels


def test_loss_rule_equals_the_recorded_float64_values(golden):
    x, sizes = golden["loss/scores"], golden["loss/sizes"]
    assert sizes.min() >= 2 and x.max() == 80.0
    loss, grad = M.np_pair_rank_loss(x, sizes, return_grad=True)
    assert abs(loss - float(golden["loss/value"])) <= 1e-12 * abs(float(golden["loss/value"]))
    assert np.abs(grad - golden["loss/grad"]).max() <= 1e-14
    # hand-written: two equal scores -> (ln 2 - 0) / ln 2 = 1, gradient (1/2 - 1, 1/2) / ln 2
    loss, grad = M.np_pair_rank_loss(np.float32([3, 3]), [2], return_grad=True)
    assert abs(loss - 1.0) < 1e-15 and np.allclose(grad, np.array([-0.5, 0.5]) / math.log(2), atol=1e-15)


def test_candidate_pairs_are_the_keys_of_the_script():
    from pyhgt_amd.sampler import candidate_pairs, _HostGraph
    node_dict = {"paper": [10, 0], "author": [40, 1]}
    g = _HostGraph((None, torch.zeros(60, dtype=torch.long), None, None, None, node_dict, {}))
    g.n_seed = {"paper": 3, "author": 6}
    name_label = [[2, 0, 1, 3], [3, 0, 1, 2], [5, 4]]
    paper_key, author_key, sizes = candidate_pairs(g, name_label)
    # the loop of train_author_disambiguation.py:280-289
    want_p = np.concatenate([np.repeat(10 + i, len(a)) for i, a in enumerate(name_label)])
    want_a = np.concatenate([np.array(a) + 40 for a in name_label])
    assert paper_key.dtype == author_key.dtype == torch.int64
    assert paper_key.tolist() == want_p.tolist() and author_key.tolist() == want_a.tolist() and sizes.tolist() == [4, 4, 2]
    with pytest.raises(IndexError):
        candidate_pairs(g, [[6], [0], [0]])
    with pytest.raises(ValueError):
        candidate_pairs(g, name_label[:2])


def test_boundary_lists_the_new_file_and_symbols():
    header = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    makefile = open(os.path.join(ROOT, "pyhgt_amd", "csrc", "Makefile")).read()
    assert "hgt_task_metrics.hip" in re.search(r"^SRCS\s*=((?:.*\\\n)*.*)", makefile, flags=re.M).group(1).split()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+HGT_ABI_VERSION\s+8\b", code) and _lib.ABI_VERSION == 8
    assert int(re.search(r"#define\s+HGT_RANK_LIST_CAP\s+(\d+)", code).group(1)) == _lib.RANK_LIST_CAP
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    import pyhgt_amd
    for name in ("rank_metrics", "pair_rank_loss", "np_rank_metrics", "np_pair_rank_loss", "candidate_pairs"):
        assert hasattr(pyhgt_amd, name)


def test_calls_without_rows_return_before_a_launch():
    lib = _lib.load()
    assert lib.hgt_rank_metrics(None, None, None, None, 0, 5, 5, 0, 0, None, None, None) == 0
    assert lib.hgt_segment_first_nll(None, None, 0, 0, None, None, None) == 0
    assert lib.hgt_segment_first_nll_bwd(None, None, 0, 0, None, None, None, None) == 0
    assert lib.hgt_rank_metrics(None, None, None, None, -1, 5, 5, 0, 0, None, None, None) == -1
    assert lib.hgt_rank_metrics(None, None, None, None, 2, 5, 5, 0, 0, None, None, None) == -1       # NULL outputs
    assert lib.hgt_segment_first_nll(None, None, 3, 8, None, None, None) == -1
