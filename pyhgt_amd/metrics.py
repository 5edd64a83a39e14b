"""Scoring a task batch: NDCG, MRR, the pair-ranking loss and the classification losses of the reference's training scripts, on the device.

After a step the scripts of the reference take one `argsort` row of the model's output at a time to the host and run `ndcg_at_k` and
`mean_reciprocal_rank` (pyHGT/utils.py:5-20) on it (OAG/train_paper_field.py:272-275, 303-308 and its siblings); the author
disambiguation script builds its loss, `mask_softmax`, from one `log_softmax` per paper (OAG/train_author_disambiguation.py:90-96).
`rank_metrics` and `pair_rank_loss` are one call each on the current stream (csrc/hgt_task_metrics.hip), without a host copy of a row.

The rule is the numpy code below, `np_rank_metrics` and `np_pair_rank_loss`; the kernels are tested against it.

Ranks.  A row is a run of C >= 0 scores s_j (float32) with relevances l_j >= 0 (float32); P of them are positive.  Ranks are 0-based
and a tie goes to the lower position (`torch.argsort(descending=True)` is not stable, so the reference leaves ties open):

    score rank of p = #{ j : s_j > s_p or (s_j == s_p and j < p) }
    ideal rank of p = #{ j : l_j > l_p or (l_j == l_p and j < p) }

Metrics.  w(0) = 1, w(i) = 1 / log2(i + 1); K = C for k=None, else k >= 1:

    DCG  = sum over the positives with rank < K of l_p * w(rank_p)
    IDCG = sum over the positives with ideal rank < K of l_p * w(ideal rank_p)
    ndcg = DCG / IDCG, 0 when IDCG == 0;    rr = 1 / (1 + min over the positives of rank_p), 0 when P == 0 (whatever k is)

A row that holds a NaN score gives NaN for both; -inf is an ordinary score.

Relevances: `labels` (float32, shaped like the scores: `ylabel` of the paper-field script), or `index` (int64 per row: l = 1 at that
column, a value outside [0, C) -- such as LabelSpace.index's -1 -- means P = 0), or neither: l = 1 at position 0 of the row (author
disambiguation: the true author comes first).  Rows: scores [n, C], or a flat [L] with `sizes`, the lengths of its consecutive rows.

Loss.  For segments of lengths l_s >= 2 over a flat score vector:

    loss = sum_s (logsumexp(seg_s) - seg_s[0]) / ln(l_s),    d loss / d s_j = g * (softmax(seg_s)_j - [j is first]) / ln(l_s)

Classification losses (`class_loss`, csrc/hgt_task_loss.hip; the rule is `np_class_loss`).  The paper-venue, ogbn-mag and paper-field
scripts put log_softmax + nll_loss (OAG/train_paper_venue.py:86, ogbn-mag/train_ogbn_mag.py:116) or KLDivLoss('batchmean')
(OAG/train_paper_field.py:87) on the Classifier's output.  Here the raw logits x [n, C] go in; logp_j = x_j - max x - log sum exp(x - max x),
and a row's term and label weight W come from one of three label forms:

    index y      term = -logp_y, W = 1;   y < 0: the row is ignored (term 0, W 0, gradient row 0);   y >= C: NaN
    labels l     term = sum over l_j > 0 of l_j (log l_j - logp_j), W = sum l_j;   an entry < 0 or NaN: NaN
    columns      [n, width] class columns, -1 = padding, distinct within a row; c = the number of entries >= 0:
                 term = -log c - (1 / c) sum logp_col = the dense form with l = 1 / c on those columns, W = 1;   c = 0: term 0, W 0;
                 an entry >= C: NaN;   with `count` (the true number of classes of a row) count > width: NaN

    d term / d x_j = W softmax(x)_j - l_j;   a NaN term has a NaN gradient row

Voted evaluation (`class_predict`, `VoteTable`, csrc/hgt_task_vote.hip; the rules are `np_class_predict` and `np_vote_add`).  The
ogbn-mag scripts report three accuracies per step, argmax of each split's rows against y (ogbn-mag/train_ogbn_mag.py:165-191), and
evaluate by vote (ogbn-mag/eval_ogbn_mag.py:128-191): every test paper owns C sums, each sampled sub-graph adds the log-probabilities
of the test papers it contains through `res.tolist()` and a dict, and the answer is the argmax of the sums.

    pred_r = np.argmax(scores_r): the lowest position among the maxima; a NaN beats every number, the first NaN wins
    row r is scored in split s iff label >= 0 and 0 <= split < n_splits (no split: s = 0); counts[s] = (scored, pred == label)
    labels / split are per-row arrays, or with `ids` tables read at ids[r]; an id outside the table is not scored
    vote: for every row whose id is in [0, n_nodes) and has a slot s: votes[s] += log_softmax(logits_r), count[s] += 1

The prediction is taken on the scores as given.  The scripts take argmax of log-probabilities; on raw logits that is the same
position except where the float32 rounding of (x - m) - ls makes the log-probabilities of two different logits equal.

Matcher retrieval (`matcher_topk`, `matcher_rank`, csrc/hgt_matcher_topk.hip; the rules are `np_matcher_scores`, `np_matcher_topk` and
`np_matcher_rank`).  With projected candidates tx [N, d] and projected queries ty [Q, d], both float32:

    s(c, q) = fl32(tx_c . ty_q accumulated in fp32) * scale, scale = the float32 nearest to 1 / sqrt(n_hid), applied once to the sum
    order of query q: scores compare as floats, -0 == +0, every NaN is one value above +inf (torch.topk's reading: a broken model
    shows); among equal scores the lower candidate position comes first
    topk: the first min(k, N) candidates of every query in that order -- values float32 [Q, k], indices int64 [Q, k], slots beyond N
    hold -inf and -1; a -0 is returned as +0 and a NaN as the quiet NaN
    rank[q] = #{ c : c comes before index[q] in the order of query q }, int64, 0-based; an index outside [0, N) gives -1

The numpy rules accumulate in float64 and round once; the kernels accumulate in fp32.  Where every product and partial sum is exact
(small integers) the two agree bit for bit; elsewhere a score differs from the rule's by at most gamma_d * sum_i |tx_ci ty_qi| * scale
with gamma_d = d 2^-24 / (1 - d 2^-24).  MRR and Hits@k follow from the ranks: mean of 1 / (1 + rank) and mean of rank < k.
"""
import numpy as np
import torch

from . import _lib

__all__ = ["Segments", "rank_metrics", "pair_rank_loss", "class_loss", "np_rank_metrics", "np_pair_rank_loss", "np_class_loss", "np_ranks",
           "class_predict", "VoteTable", "np_class_predict", "np_vote_add", "np_matcher_scores", "np_matcher_topk", "np_matcher_rank",
           "matcher_scale", "matcher_topk", "matcher_rank"]


# ---------------------------------------------------------------------------------------------------------------- the rule
def matcher_scale(n_hid):
    """the float32 nearest to 1 / sqrt(n_hid): the scale of the Matcher's scores"""
    return np.float32(1.0 / np.sqrt(np.float64(n_hid)))


def np_matcher_scores(tx, ty, scale):
    """s [N, Q] float32: fl32(tx @ ty^T, accumulated in float64) * scale in float32"""
    tx, ty = np.asarray(tx, dtype=np.float32), np.asarray(ty, dtype=np.float32)
    if tx.ndim != 2 or ty.ndim != 2 or tx.shape[1] != ty.shape[1]:
        raise ValueError("pyhgt_amd: tx is [N, d] and ty is [Q, d]")
    with np.errstate(invalid="ignore", over="ignore"):
        dot = (tx.astype(np.float64) @ ty.astype(np.float64).T).astype(np.float32)
        return (dot * np.float32(scale)).astype(np.float32)


def _np_order_image(s):
    """int64 image of float32 scores that sorts like the order of the module docstring: -0 == +0, every NaN one value above +inf"""
    s = np.where(np.isnan(s), np.float32(np.nan), s.astype(np.float32) + np.float32(0.0))      # one NaN; -0 + 0 = +0
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.int64)
    u = np.where(np.isnan(s), 0x7FC00000, u)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def np_matcher_topk(tx, ty, k, scale):
    """(values float32 [Q, k], indices int64 [Q, k]): the rule of the module docstring"""
    if int(k) != k or k < 1:
        raise ValueError("pyhgt_amd: k is an integer >= 1")
    k = int(k)
    s = np_matcher_scores(tx, ty, scale)
    N, Q = s.shape
    values = np.full((Q, k), -np.inf, np.float32)
    indices = np.full((Q, k), -1, np.int64)
    m = min(k, N)
    for q in range(Q):
        order = np.argsort(-_np_order_image(s[:, q]), kind="stable")[:m]
        col = s[order, q]
        values[q, :m] = np.where(np.isnan(col), np.float32(np.nan), col + np.float32(0.0))
        indices[q, :m] = order
    return values, indices


def np_matcher_rank(tx, ty, index, scale):
    """rank int64 [Q]: how many candidates come before index[q] in the order of query q; -1 for an index outside [0, N)"""
    s = np_matcher_scores(tx, ty, scale)
    N, Q = s.shape
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    if index.size != Q:
        raise ValueError("pyhgt_amd: one index per query")
    rank = np.full(Q, -1, np.int64)
    for q in range(Q):
        t = int(index[q])
        if 0 <= t < N:
            img = _np_order_image(s[:, q])
            rank[q] = int(np.sum(img > img[t])) + int(np.sum(img[:t] == img[t]))
    return rank


def np_ranks(values):
    """0-based descending ranks of a 1-d array, a tie to the lower position (-0.0 == 0.0, as everywhere in IEEE comparisons)"""
    values = np.asarray(values)
    order = np.argsort(-values, kind="stable")
    ranks = np.empty(values.size, np.int64)
    ranks[order] = np.arange(values.size)
    return ranks


def _np_row(s, l, k):
    if np.isnan(s).any():
        return np.nan, np.nan
    pos = np.flatnonzero(l > 0)
    if pos.size == 0:
        return 0.0, 0.0
    K = s.size if k is None else k
    rel = l[pos].astype(np.float64)

    def dcg(rank):
        w = np.ones(rank.size)
        w[rank > 0] = 1.0 / np.log2(rank[rank > 0] + 1.0)
        return float(np.sum((rel * w)[rank < K]))

    rank = np_ranks(s)[pos]
    ideal = dcg(np_ranks(np.where(l > 0, l, 0))[pos])
    return (dcg(rank) / ideal if ideal else 0.0), 1.0 / (1.0 + int(rank.min()))


def _check_k(k):
    if k is not None and (int(k) != k or k < 1):
        raise ValueError("pyhgt_amd: k is None or an integer >= 1")
    return None if k is None else int(k)


def _np_sizes(sizes, total, least):
    sizes = np.asarray(sizes if not isinstance(sizes, Segments) else sizes.sizes, dtype=np.int64).reshape(-1)
    if sizes.size and sizes.min() < least:
        raise ValueError("pyhgt_amd: a segment shorter than %d" % least)
    if int(sizes.sum()) != total:
        raise ValueError("pyhgt_amd: sizes add up to %d, the scores have %d entries" % (int(sizes.sum()), total))
    return sizes


def np_rank_metrics(scores, labels=None, index=None, k=None, sizes=None):
    """(ndcg, rr), float64 arrays of one value per row: the definition of this module's docstring in numpy"""
    k = _check_k(k)
    if labels is not None and index is not None:
        raise ValueError("pyhgt_amd: labels or index, not both")
    scores = np.asarray(scores, dtype=np.float32)
    if sizes is None:
        if scores.ndim != 2:
            raise ValueError("pyhgt_amd: scores are [n, C], or flat with sizes")
        rows = [(r * scores.shape[1], scores.shape[1]) for r in range(scores.shape[0])]
    else:
        if scores.ndim != 1:
            raise ValueError("pyhgt_amd: with sizes the scores are flat")
        sizes = _np_sizes(sizes, scores.size, 0)
        rows = list(zip(np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist(), sizes.tolist())) if sizes.size else []
    flat = scores.reshape(-1)
    if labels is not None:
        labels = np.asarray(labels, dtype=np.float32)
        if labels.shape != scores.shape:
            raise ValueError("pyhgt_amd: labels are shaped like the scores")
        labels = labels.reshape(-1)
    if index is not None:
        index = np.asarray(index, dtype=np.int64).reshape(-1)
        if index.size != len(rows):
            raise ValueError("pyhgt_amd: one index per row")
    ndcg, rr = np.zeros(len(rows)), np.zeros(len(rows))
    for r, (beg, c) in enumerate(rows):
        s = flat[beg:beg + c]
        if labels is not None:
            l = labels[beg:beg + c]
        else:
            l = np.zeros(c, np.float32)
            t = 0 if index is None else int(index[r])
            if 0 <= t < c:
                l[t] = 1.0
        ndcg[r], rr[r] = _np_row(s, l, k)
    return ndcg, rr


def np_pair_rank_loss(scores, sizes, return_grad=False):
    """the loss of this module's docstring in float64 on the scores as given; with return_grad also d loss / d scores (g = 1)"""
    x = np.asarray(scores).astype(np.float64).reshape(-1)
    sizes = _np_sizes(sizes, x.size, 2)
    loss, grad, beg = 0.0, np.zeros_like(x), 0
    for l in sizes.tolist():
        seg = x[beg:beg + l]
        m = seg.max()
        e = np.exp(seg - m)
        loss += (m + np.log(e.sum()) - seg[0]) / np.log(l)
        grad[beg:beg + l] = e / e.sum() / np.log(l)
        grad[beg] -= 1.0 / np.log(l)
        beg += l
    return (loss, grad) if return_grad else loss


def _one_label_form(labels, index, columns, count):
    if (labels is not None) + (index is not None) + (columns is not None) != 1:
        raise ValueError("pyhgt_amd: exactly one of labels, index and columns")
    if count is not None and columns is None:
        raise ValueError("pyhgt_amd: count goes with columns")


def np_class_loss(logits, labels=None, index=None, columns=None, count=None, return_grad=False):
    """the per-row terms of this module's docstring in float64 on the logits as given: float64 [n]; with return_grad also
    d(sum of the terms) / d logits, float64 [n, C]"""
    _one_label_form(labels, index, columns, count)
    x = np.asarray(logits).astype(np.float64)
    if x.ndim != 2:
        raise ValueError("pyhgt_amd: logits are [n, C]")
    n, C = x.shape
    if labels is not None:
        labels = np.asarray(labels).astype(np.float64)
        if labels.shape != x.shape:
            raise ValueError("pyhgt_amd: labels are shaped like the logits")
    if index is not None:
        index = np.asarray(index, dtype=np.int64).reshape(-1)
        if index.size != n:
            raise ValueError("pyhgt_amd: one index per row")
    if columns is not None:
        columns = np.asarray(columns, dtype=np.int64)
        if columns.ndim != 2 or columns.shape[0] != n or columns.shape[1] < 1:
            raise ValueError("pyhgt_amd: columns are [n, width >= 1]")
        if count is not None:
            count = np.asarray(count, dtype=np.int64).reshape(-1)
            if count.size != n:
                raise ValueError("pyhgt_amd: one count per row")
    terms, grad = np.zeros(n), np.zeros((n, C))
    with np.errstate(all="ignore"):
        for r in range(n):
            m = x[r].max() if C else -np.inf
            e = np.exp(x[r] - m)
            logp = x[r] - m - np.log(e.sum())
            p, l, W = e / e.sum(), np.zeros(C), 0.0
            if index is not None:
                y = int(index[r])
                if y >= C:
                    W = np.nan
                elif y >= 0:
                    l[y], W, terms[r] = 1.0, 1.0, -logp[y]
            elif labels is not None:
                l = labels[r]
                pos = l > 0
                W = np.nan if not (l >= 0).all() else float(l[pos].sum())
                terms[r] = float(np.sum(l[pos] * (np.log(l[pos]) - logp[pos])))
            else:
                ent = columns[r][columns[r] >= 0]
                if (ent >= C).any() or (count is not None and count[r] > columns.shape[1]):
                    W = np.nan
                elif ent.size:
                    l[ent], W = 1.0 / ent.size, 1.0
                    terms[r] = -np.log(ent.size) - float(np.sum(logp[ent])) / ent.size
            if np.isnan(W):
                terms[r], grad[r] = np.nan, np.nan
            elif W != 0 or labels is not None:
                grad[r] = W * p - l
    return (terms, grad) if return_grad else terms


def np_class_predict(scores, labels=None, split=None, n_splits=1, ids=None):
    """pred (int64 [n]) = np.argmax of every row of scores [n, C >= 1]; with `labels` also counts (int32 [n_splits, 2]): per split
    the rows scored and those with pred == label, by the rule of this module's docstring.  labels (and split) hold one entry per row,
    or with `ids` (one id per row) one entry per node of a table, read at the id."""
    scores = np.asarray(scores)
    if scores.ndim != 2 or (scores.shape[0] and scores.shape[1] < 1):
        raise ValueError("pyhgt_amd: scores are [n, C >= 1]")
    n = scores.shape[0]
    pred = np.argmax(scores, axis=1).astype(np.int64) if n else np.zeros(0, np.int64)
    if labels is None:
        if split is not None:
            raise ValueError("pyhgt_amd: split goes with labels")
        return pred
    n_splits = _check_splits(split, n_splits)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    split = np.zeros(labels.size, np.int64) if split is None else np.asarray(split, dtype=np.int64).reshape(-1)
    if split.size != labels.size:
        raise ValueError("pyhgt_amd: one split id per label")
    if ids is None:
        if labels.size != n:
            raise ValueError("pyhgt_amd: one label per row, or a table with ids")
        y, s = labels, split
    else:
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if ids.size != n:
            raise ValueError("pyhgt_amd: one id per row")
        inside = (ids >= 0) & (ids < labels.size)
        at = np.where(inside, ids, 0)
        y = np.where(inside, labels[at], -1) if labels.size else np.full(n, -1, np.int64)
        s = np.where(inside, split[at], -1) if labels.size else np.full(n, -1, np.int64)
    scored = (y >= 0) & (s >= 0) & (s < n_splits)
    counts = np.zeros((n_splits, 2), np.int32)
    np.add.at(counts[:, 0], s[scored], 1)
    np.add.at(counts[:, 1], s[scored & (pred == y)], 1)
    return pred, counts


def _check_splits(split, n_splits):
    if int(n_splits) != n_splits or not 1 <= n_splits <= (_lib.PREDICT_MAX_SPLITS if split is not None else 1):
        raise ValueError("pyhgt_amd: 1 <= n_splits <= %d with split, 1 without" % _lib.PREDICT_MAX_SPLITS)
    return int(n_splits)


def _piece_ptr(piece_sizes, n):
    """host offsets (int32 [B + 1]) of the pieces of n rows; None: one piece"""
    sizes = np.asarray([n] if piece_sizes is None else piece_sizes, dtype=np.int64).reshape(-1)
    if sizes.size and sizes.min() < 0:
        raise ValueError("pyhgt_amd: a negative piece size")
    if int(sizes.sum()) != n:
        raise ValueError("pyhgt_amd: the piece sizes add up to %d, there are %d rows" % (int(sizes.sum()), n))
    if n >= 2 ** 31:
        raise ValueError("pyhgt_amd: too many rows")
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def np_vote_add(votes, count, slot_of, logits, ids, piece_sizes=None):
    """The vote of eval_ogbn_mag.py:148-150 / 177-179 in float64, in place on a numpy table: votes float64 [n_slots, C], count an
    integer array [n_slots], slot_of [n_nodes] (-1 = no slot).  For every row of logits [n, C] whose id lies in [0, n_nodes) and has
    a slot s in [0, n_slots): votes[s] += log_softmax(row), count[s] += 1; the pieces (consecutive runs of `piece_sizes` rows, None =
    one) are added in order.  ValueError if a piece holds a slotted node twice: the device path has one writer per slot and launch."""
    if not isinstance(votes, np.ndarray) or votes.dtype != np.float64 or votes.ndim != 2:
        raise TypeError("pyhgt_amd: votes is a float64 numpy array [n_slots, C]")
    if not isinstance(count, np.ndarray) or count.dtype.kind != "i" or count.shape != votes.shape[:1]:
        raise TypeError("pyhgt_amd: count is an integer numpy array [n_slots]")
    x = np.asarray(logits).astype(np.float64)
    if x.ndim != 2 or x.shape[1] != votes.shape[1]:
        raise ValueError("pyhgt_amd: logits are [n, C] with the table's C")
    slot_of = np.asarray(slot_of, dtype=np.int64).reshape(-1)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.size != x.shape[0]:
        raise ValueError("pyhgt_amd: one id per row")
    ptr = _piece_ptr(piece_sizes, x.shape[0])
    inside = (ids >= 0) & (ids < slot_of.size)
    slot = np.where(inside, slot_of[np.where(inside, ids, 0)], -1) if slot_of.size else np.full(ids.size, -1, np.int64)
    has = (slot >= 0) & (slot < votes.shape[0])
    for b in range(ptr.size - 1):
        rows = np.arange(ptr[b], ptr[b + 1])[has[ptr[b]:ptr[b + 1]]]
        if np.unique(slot[rows]).size != rows.size:
            raise ValueError("pyhgt_amd: piece %d holds a node with a slot more than once" % b)
    with np.errstate(all="ignore"):
        m = x.max(axis=1, keepdims=True) if x.size else x
        logp = x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True)) if x.size else x
    for b in range(ptr.size - 1):
        rows = np.arange(ptr[b], ptr[b + 1])[has[ptr[b]:ptr[b + 1]]]
        votes[slot[rows]] += logp[rows]
        count[slot[rows]] += 1


# ---------------------------------------------------------------------------------------------------------------- the device calls
class Segments:
    """The rows of a flat score vector: `sizes` (a host sequence, `key_size` of the author script) with their offsets as an int64
    device tensor, built once and good for any number of rank_metrics / pair_rank_loss calls on that device."""

    def __init__(self, sizes, device=None):
        self.sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
        if self.sizes.size and self.sizes.min() < 0:
            raise ValueError("pyhgt_amd: a negative segment size")
        self.n, self.total = int(self.sizes.size), int(self.sizes.sum())
        self.longest, self.shortest = (int(self.sizes.max()), int(self.sizes.min())) if self.n else (0, 0)
        if self.n >= 2 ** 31 or self.longest >= 2 ** 31 - 1024:
            raise ValueError("pyhgt_amd: too many or too long segments")
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.row_ptr = None
        if self.device is not None and self.device.type == "cuda":
            self.row_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)).to(self.device)

    @classmethod
    def of(cls, sizes, like):
        if isinstance(sizes, cls):
            if like.is_cuda and (sizes.device is None or sizes.device != like.device):
                raise ValueError("pyhgt_amd: the Segments were built for %s, the scores are on %s" % (sizes.device, like.device))
            return sizes
        return cls(sizes, like.device)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


_ptr = _lib.ptr


def _rows_f32(t, what):
    """a float32 device tensor whose last dimension has unit stride (a column slice of a wider tensor stays as it is)"""
    if t.dtype != torch.float32:
        raise TypeError("pyhgt_amd: %s must be float32, got %s" % (what, t.dtype))
    if t.dim() == 2 and t.size(0) > 0 and t.size(1) > 0 and (t.stride(1) != 1 and t.size(1) > 1 or t.stride(0) < t.size(1)):
        t = t.contiguous()
    elif t.dim() == 1 and t.numel() > 1 and t.stride(0) != 1:
        t = t.contiguous()
    return t


def rank_metrics(scores, labels=None, index=None, k=None, sizes=None):
    """(ndcg, rr) of every row: float64 tensors on the scores' device, one value per row (the definitions are in the module docstring).
    scores: float32 [n, C] with unit column stride -- a column slice of a wider tensor is read in place -- or, with `sizes` (a host
    sequence or a `Segments`), a flat float32 [L].  labels: float32 shaped like the scores; index: integers, one per row; neither: the
    first position of every row is the positive.  One call of hgt_rank_metrics on the current stream, no synchronisation.  On CPU
    tensors the result is np_rank_metrics's."""
    k = _check_k(k)
    if not isinstance(scores, torch.Tensor):
        raise TypeError("pyhgt_amd: scores must be a torch tensor")
    if scores.dtype != torch.float32:
        raise TypeError("pyhgt_amd: scores must be float32, got %s" % scores.dtype)
    if labels is not None and index is not None:
        raise ValueError("pyhgt_amd: labels or index, not both")
    if not scores.is_cuda:
        host = lambda t: None if t is None else torch.as_tensor(t).detach().cpu().numpy()
        ndcg, rr = np_rank_metrics(scores.detach().numpy(), host(labels), host(index), k, sizes)
        return torch.from_numpy(ndcg), torch.from_numpy(rr)
    scores = scores.detach()
    if sizes is None:
        if scores.dim() != 2:
            raise ValueError("pyhgt_amd: scores are [n, C], or flat with sizes")
        seg, (n, n_cols) = None, scores.shape
        if n_cols >= 2 ** 31 - 1024 or n >= 2 ** 31:
            raise ValueError("pyhgt_amd: too many rows or columns")
    else:
        if scores.dim() != 1:
            raise ValueError("pyhgt_amd: with sizes the scores are flat")
        seg = Segments.of(sizes, scores)
        if seg.total != scores.numel():
            raise ValueError("pyhgt_amd: sizes add up to %d, the scores have %d entries" % (seg.total, scores.numel()))
        n, n_cols = seg.n, seg.longest
    scores = _rows_f32(scores, "scores")
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.device != scores.device or labels.shape != scores.shape:
            raise ValueError("pyhgt_amd: labels are a tensor shaped like the scores, on their device")
        labels = _rows_f32(labels.detach(), "labels")
    if index is not None:
        index = torch.as_tensor(index, device=scores.device).reshape(-1).to(torch.int64).contiguous()
        if index.numel() != n:
            raise ValueError("pyhgt_amd: one index per row")
    ndcg = torch.empty(n, dtype=torch.float64, device=scores.device)
    rr = torch.empty(n, dtype=torch.float64, device=scores.device)
    ld = lambda t: 0 if t is None or t.dim() != 2 else max(int(t.stride(0)), n_cols)
    with torch.cuda.device(scores.device):
        _lib.check(_lib.load().hgt_rank_metrics(_ptr(scores), _ptr(labels), _ptr(index), None if seg is None else seg.row_ptr.data_ptr(), n,
                                                n_cols, ld(scores), ld(labels), 0 if k is None else min(k, 2 ** 31 - 1), _ptr(ndcg), _ptr(rr),
                                                _stream(scores)), "hgt_rank_metrics")
    return ndcg, rr


class _PairRankLoss(torch.autograd.Function):
    """per-segment losses [n] of a flat float32 score vector (hgt_segment_first_nll / _bwd)"""

    @staticmethod
    def forward(ctx, scores, seg):
        x = scores.detach().contiguous()
        loss = torch.empty(seg.n, dtype=torch.float32, device=x.device)
        lse = torch.empty(seg.n, 2, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().hgt_segment_first_nll(_ptr(x), seg.row_ptr.data_ptr(), seg.n, seg.longest, _ptr(loss), _ptr(lse), _stream(x)),
                       "hgt_segment_first_nll")
        ctx.save_for_backward(x, lse)
        ctx.seg = seg
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        x, lse = ctx.saved_tensors
        seg = ctx.seg
        g = grad_loss.detach().float().contiguous()
        grad = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().hgt_segment_first_nll_bwd(_ptr(x), seg.row_ptr.data_ptr(), seg.n, seg.longest, _ptr(lse), _ptr(g), _ptr(grad),
                                                             _stream(x)), "hgt_segment_first_nll_bwd")
        return grad, None


def pair_rank_loss(scores, sizes, reduce=True):
    """The pair-ranking loss of the author-disambiguation script (`mask_softmax`): scores flat float32 [L] on the device -- the output
    of Matcher(pair=True) -- and `sizes`, a host sequence (`key_size`) or a `Segments`, every one >= 2 (ValueError otherwise: the
    reference divides by log 1 = 0 there).  Differentiable; forward and backward are one call each on the current stream, without
    atomics, so the result is the same bits every time.  reduce=False returns the per-segment terms [n] instead of their sum."""
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32:
        raise TypeError("pyhgt_amd: scores must be a float32 tensor")
    if scores.dim() != 1:
        raise ValueError("pyhgt_amd: the scores are flat")
    if not scores.is_cuda:
        raise RuntimeError("pyhgt_amd: pair_rank_loss runs only on a ROCm GPU tensor; np_pair_rank_loss is the definition on the host")
    seg = Segments.of(sizes, scores)
    if seg.n and seg.shortest < 2:
        raise ValueError("pyhgt_amd: a segment shorter than 2")
    if seg.total != scores.numel():
        raise ValueError("pyhgt_amd: sizes add up to %d, the scores have %d entries" % (seg.total, scores.numel()))
    if seg.n == 0:
        terms = scores.new_zeros(0) + scores.sum() * 0
    else:
        terms = _PairRankLoss.apply(scores, seg)
    return terms.sum() if reduce else terms


class _ClassLoss(torch.autograd.Function):
    """per-row terms [n] and label weights [n] of float32 logits [n, C] (hgt_class_loss / _bwd); the labels are constants"""

    @staticmethod
    def forward(ctx, logits, labels, index, columns, count):
        x = _rows_f32(logits.detach(), "logits")
        n, n_cols = x.shape
        loss = torch.empty(n, dtype=torch.float32, device=x.device)
        lse = torch.empty(n, 2, dtype=torch.float32, device=x.device)
        wsum = torch.empty(n, dtype=torch.float32, device=x.device)
        ld = lambda t: 0 if t is None else max(int(t.stride(0)), n_cols)
        ctx.call = (_ptr(x), ld(x), n, n_cols, _ptr(labels), ld(labels), _ptr(index), _ptr(columns), 0 if columns is None else columns.size(1),
                    _ptr(count))
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().hgt_class_loss(*ctx.call, _ptr(loss), _ptr(lse), _ptr(wsum), _stream(x)), "hgt_class_loss")
        ctx.save_for_backward(x, lse, wsum, *(t for t in (labels, index, columns, count) if t is not None))
        ctx.mark_non_differentiable(wsum)
        return loss, wsum

    @staticmethod
    def backward(ctx, grad_loss, _):
        x, lse, wsum = ctx.saved_tensors[:3]
        g = grad_loss.detach().float().contiguous()
        grad = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().hgt_class_loss_bwd(*ctx.call, _ptr(lse), _ptr(wsum), _ptr(g), _ptr(grad), x.size(1), _stream(x)),
                       "hgt_class_loss_bwd")
        return grad, None, None, None, None


def class_loss(logits, labels=None, index=None, columns=None, count=None, reduce="mean"):
    """The classification losses of the paper-venue / ogbn-mag scripts (`index`: log_softmax + NLLLoss) and of the paper-field script
    (`labels`, or the same distribution as `columns` [n, width] with -1 padding and optionally `count`, as LabelSpace.columns gives
    them: log_softmax + KLDivLoss) on the raw logits: float32 [n, C] on the device with unit column stride -- a column slice of a wider
    tensor is read in place.  Differentiable in the logits; forward and backward are one call each on the current stream, without
    atomics, so the result is the same bits every time.  reduce: "mean" = NLLLoss() for `index` (the sum over the rows with
    index >= 0 divided by their number, NaN without one) and 'batchmean' (sum / n) for `labels` / `columns`; "sum"; None = the
    per-row terms [n] of the module docstring."""
    _one_label_form(labels, index, columns, count)
    if reduce not in ("mean", "sum", None):
        raise ValueError("pyhgt_amd: reduce is 'mean', 'sum' or None")
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32:
        raise TypeError("pyhgt_amd: logits must be a float32 tensor")
    if labels is not None and (not isinstance(labels, torch.Tensor) or labels.dtype != torch.float32):
        raise TypeError("pyhgt_amd: labels must be a float32 tensor")
    if logits.dim() != 2:
        raise ValueError("pyhgt_amd: logits are [n, C]")
    if not logits.is_cuda:
        raise RuntimeError("pyhgt_amd: class_loss runs only on a ROCm GPU tensor; np_class_loss is the definition on the host")
    n, n_cols = logits.shape
    if n_cols >= 2 ** 31 - 1024 or n >= 2 ** 31:
        raise ValueError("pyhgt_amd: too many rows or columns")
    integers = lambda t, dtype: torch.as_tensor(t, device=logits.device).to(dtype).contiguous()
    if labels is not None:
        if labels.device != logits.device or labels.shape != logits.shape:
            raise ValueError("pyhgt_amd: labels are a tensor shaped like the logits, on their device")
        labels = _rows_f32(labels.detach(), "labels")
    if index is not None:
        index = integers(index, torch.int64).reshape(-1)
        if index.numel() != n:
            raise ValueError("pyhgt_amd: one index per row")
    if columns is not None:
        columns = integers(columns, torch.int32)
        if columns.dim() != 2 or columns.size(0) != n or columns.size(1) < 1:
            raise ValueError("pyhgt_amd: columns are [n, width >= 1]")
        if count is not None:
            count = integers(count, torch.int32).reshape(-1)
            if count.numel() != n:
                raise ValueError("pyhgt_amd: one count per row")
    if n == 0:
        terms, wsum = logits.new_zeros(0) + logits.sum() * 0, logits.new_zeros(0)
    else:
        terms, wsum = _ClassLoss.apply(logits, labels, index, columns, count)
    if reduce is None:
        return terms
    if reduce == "sum":
        return terms.sum()
    return terms.sum() / (wsum.sum() if index is not None else terms.new_tensor(float(n)))


def _ids_i64(t, n, device, what):
    t = torch.as_tensor(t, device=device).reshape(-1)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("pyhgt_amd: %s must be integers, got %s" % (what, t.dtype))
    if n is not None and t.numel() != n:
        raise ValueError("pyhgt_amd: %s has %d entries, expected %d" % (what, t.numel(), n))
    return t.to(torch.int64).contiguous()


def class_predict(scores, labels=None, split=None, n_splits=1, ids=None):
    """pred = argmax of every row of scores (float32 [n, C >= 1] on the device with unit column stride; a column slice of a wider tensor
    is read in place), as np.argmax takes it: int64 [n].  With `labels` (integers) also counts, int32 [n_splits, 2] on the device: per
    split the rows scored and the rows with pred == label -- the three accuracies of a step of train_ogbn_mag.py:165-191 are
    counts[:, 1] / counts[:, 0].  A row is scored iff label >= 0 and 0 <= split < n_splits (`split`: int32 ids; None: everything in
    split 0).  labels / split hold one entry per row; with `ids` (int64 [n]) they are resident tables -- graph.y and the split id of
    every node -- read at ids[r], and an id outside the table is not scored.  One call of hgt_class_predict on the current stream, no
    synchronisation, no [n, C] temporary; the definition is np_class_predict."""
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32:
        raise TypeError("pyhgt_amd: scores must be a float32 tensor")
    if scores.dim() != 2 or (scores.size(0) and scores.size(1) < 1):
        raise ValueError("pyhgt_amd: scores are [n, C >= 1]")
    if split is not None and labels is None:
        raise ValueError("pyhgt_amd: split goes with labels")
    if ids is not None and labels is None:
        raise ValueError("pyhgt_amd: ids go with labels")
    n_splits = _check_splits(split, n_splits)
    for what, t in (("labels", labels), ("split", split), ("ids", ids)):
        if isinstance(t, torch.Tensor) and (t.dtype.is_floating_point or t.dtype == torch.bool):
            raise TypeError("pyhgt_amd: %s must be integers, got %s" % (what, t.dtype))
    if not scores.is_cuda:
        raise RuntimeError("pyhgt_amd: class_predict runs only on a ROCm GPU tensor; np_class_predict is the definition on the host")
    n, n_cols = scores.shape
    if n_cols >= 2 ** 31 - 1024 or n >= 2 ** 31:
        raise ValueError("pyhgt_amd: too many rows or columns")
    x = _rows_f32(scores.detach(), "scores")
    dev, n_table, counts = x.device, 0, None
    if labels is not None:
        if ids is not None:
            ids = _ids_i64(ids, n, dev, "ids")
        labels = _ids_i64(labels, n if ids is None else None, dev, "labels")
        n_table = labels.numel()
        if split is not None:
            split = _ids_i64(split, n_table, dev, "split").to(torch.int32)
        counts = (torch.zeros if n == 0 or n_table == 0 else torch.empty)(n_splits, 2, dtype=torch.int32, device=dev)
    pred = torch.empty(n, dtype=torch.int64, device=dev)
    if n:
        tables = (_ptr(ids), n_table, _ptr(labels), _ptr(split), n_splits) if n_table else (None, 0, None, None, 1)      # (no label: no scoring)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().hgt_class_predict(x.data_ptr(), max(int(x.stride(0)), n_cols), n, n_cols, *tables, pred.data_ptr(),
                                                     counts.data_ptr() if n_table else None, _stream(x)), "hgt_class_predict")
    return pred if labels is None else (pred, counts)


class VoteTable:
    """The sums of a voted evaluation (eval_ogbn_mag.py:110, 128-191) on the device.  `nodes`: the int64 ids that own a slot, e.g. the
    test papers; slot i belongs to nodes[i]; None: every one of the n_nodes nodes.  Duplicate entries raise ValueError.
    .votes float32 [n_slots, n_classes] (zeros), .count int32 [n_slots], .slot_of int32 [n_nodes] (-1 = no slot), .nodes int64.
    `.votes` may be replaced by a column slice (unit column stride) of a wider float32 tensor: its other columns are left alone."""

    def __init__(self, n_nodes, n_classes, nodes=None, device=None):
        n_nodes, n_classes = int(n_nodes), int(n_classes)
        if n_nodes < 0 or n_classes < 1 or n_classes >= 2 ** 31 - 1024:
            raise ValueError("pyhgt_amd: n_nodes >= 0 and 1 <= n_classes < 2^31 - 1024")
        if nodes is None:
            host = np.arange(n_nodes, dtype=np.int64)
        else:
            host = (nodes.detach().cpu().numpy() if isinstance(nodes, torch.Tensor) else np.asarray(nodes)).reshape(-1)
            if host.dtype.kind not in "iu":
                raise TypeError("pyhgt_amd: nodes are integer ids")
            host = host.astype(np.int64)
            if host.size and (host.min() < 0 or host.max() >= n_nodes):
                raise ValueError("pyhgt_amd: nodes outside [0, %d)" % n_nodes)
            if np.unique(host).size != host.size:
                raise ValueError("pyhgt_amd: a node is listed twice")
        if host.size >= 2 ** 31:
            raise ValueError("pyhgt_amd: too many slots")
        slot_of = np.full(n_nodes, -1, np.int32)
        slot_of[host] = np.arange(host.size, dtype=np.int32)
        self.n_nodes, self.n_classes, self.n_slots = n_nodes, n_classes, int(host.size)
        self.device = torch.device("cpu" if device is None else device)
        self.nodes = torch.from_numpy(host).to(self.device)
        self.slot_of = torch.from_numpy(slot_of).to(self.device)
        self.votes = torch.zeros(self.n_slots, n_classes, dtype=torch.float32, device=self.device)
        self.count = torch.zeros(self.n_slots, dtype=torch.int32, device=self.device)

    def reset(self):
        self.votes.zero_()
        self.count.zero_()

    def add(self, logits, ids, piece_sizes=None, check=False):
        """votes[slot_of[ids[r]]] += log_softmax(logits[r]), count += 1, for every row whose id has a slot: raw logits float32 [n, C] on
        the table's device, ids int64 [n].  piece_sizes: a host sequence of row counts, e.g. the papers of each piece of a stack (None:
        one piece); one launch per piece, in order.  Within a piece the slotted ids must be distinct (a sampled sub-graph holds a node
        once); check=True verifies that with one host read and raises ValueError.  No atomics: the same calls give the same bits."""
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32:
            raise TypeError("pyhgt_amd: logits must be a float32 tensor")
        if logits.dim() != 2 or logits.size(1) != self.n_classes:
            raise ValueError("pyhgt_amd: logits are [n, %d]" % self.n_classes)
        if not logits.is_cuda or not self.votes.is_cuda:
            raise RuntimeError("pyhgt_amd: VoteTable.add runs only on a ROCm GPU tensor and table; np_vote_add is the definition on the host")
        if logits.device != self.votes.device:
            raise ValueError("pyhgt_amd: the logits are on %s, the table on %s" % (logits.device, self.votes.device))
        n = logits.size(0)
        ids = _ids_i64(ids, n, logits.device, "ids")
        ptr = _piece_ptr(piece_sizes, n)
        if n == 0:
            return self
        if check:
            inside = (ids >= 0) & (ids < self.n_nodes)
            slot = torch.where(inside, self.slot_of[torch.where(inside, ids, 0)].long(), -1) if self.n_nodes else torch.full_like(ids, -1)
            piece = torch.repeat_interleave(torch.arange(ptr.size - 1, device=ids.device), torch.from_numpy(np.diff(ptr)).to(ids.device),
                                            output_size=n)
            key = torch.where(slot >= 0, piece * max(self.n_slots, 1) + slot, -1 - torch.arange(n, device=ids.device)).sort().values
            if bool((key[1:] == key[:-1]).any()):
                raise ValueError("pyhgt_amd: a piece holds a node with a slot more than once")
        x = _rows_f32(logits.detach(), "logits")
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().hgt_vote_add(x.data_ptr(), max(int(x.stride(0)), self.n_classes), self.n_classes, ids.data_ptr(),
                                                ptr.ctypes.data, int(ptr.size - 1), _ptr(self.slot_of), self.n_nodes, _ptr(self.votes),
                                                max(int(self.votes.stride(0)), self.n_classes), _ptr(self.count), self.n_slots, _stream(x)),
                       "hgt_vote_add")
        return self

    def predict(self, labels=None):
        """pred int64 [n_slots]: the argmax of every slot's sums, -1 for a slot that was never voted on.  With `labels` (one per slot,
        < 0 = not scored) also a device int32 pair (n_voted, n_correct) over the voted slots.  One hgt_class_predict launch on
        .votes; the slots of zero count are left out through its `split`."""
        if not self.votes.is_cuda:
            raise RuntimeError("pyhgt_amd: VoteTable.predict runs only on a ROCm GPU table; np_class_predict is the definition on the host")
        voted = self.count > 0
        if labels is None:
            return torch.where(voted, class_predict(self.votes), -1)
        pred, counts = class_predict(self.votes, labels=labels, split=voted.to(torch.int32) - 1, n_splits=1)
        return torch.where(voted, pred, -1), counts[0]

    def accuracy(self, labels):
        """the share of the voted (and labelled) slots whose prediction equals its label: a Python float after one host read"""
        n_voted, n_correct = self.predict(labels)[1].tolist()
        return n_correct / n_voted if n_voted else float("nan")


# ---------------------------------------------------------------------------------------------------------------- matcher retrieval
def _matcher_args(tx, ty, what):
    for t, name in ((tx, "tx"), (ty, "ty")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
            raise TypeError("pyhgt_amd: %s: %s must be a float32 [rows, d] tensor" % (what, name))
    if not tx.is_cuda or not ty.is_cuda:
        raise RuntimeError("pyhgt_amd: %s runs only on ROCm GPU tensors; np_%s is the definition on the host" % (what, what))
    if tx.device != ty.device:
        raise ValueError("pyhgt_amd: %s: tx is on %s, ty on %s" % (what, tx.device, ty.device))
    if tx.size(1) != ty.size(1):
        raise ValueError("pyhgt_amd: %s: tx has %d columns, ty has %d" % (what, tx.size(1), ty.size(1)))
    tx, ty = _rows_f32(tx.detach(), "tx"), _rows_f32(ty.detach(), "ty")
    ld = lambda t: max(int(t.stride(0)), int(t.size(1))) if t.size(0) > 1 else int(t.size(1))
    return tx, ty, ld(tx), ld(ty)


def _matcher_scratch(lib, n, q, k, chunk_rows, device):
    nb = _lib.C.c_uint64()
    _lib.check(lib.hgt_matcher_topk_bytes(n, q, k, chunk_rows, _lib.C.byref(nb)), "hgt_matcher_topk_bytes")
    return torch.empty(int(nb.value), dtype=torch.uint8, device=device)


def matcher_topk(tx, ty, k, scale, chunk_rows=0):
    """(values float32 [Q, k], indices int64 [Q, k]) of the scores (tx @ ty^T) * scale without the [N, Q] matrix: the rule is
    np_matcher_topk (module docstring).  tx [N, d], ty [Q, d]: float32 device tensors with unit column stride (row slices and column
    slices of wider tensors are read in place); d % 4 == 0, d <= 1024, 1 <= k <= _lib.TOPK_MAX_K.  chunk_rows > 0 fixes the length of
    the candidate chunks (the result does not depend on it).  Two launches on the current stream, no synchronisation."""
    tx, ty, ldx, ldy = _matcher_args(tx, ty, "matcher_topk")
    if int(k) != k or k < 1 or k > 2 ** 31 - 1:
        raise ValueError("pyhgt_amd: k is an integer >= 1")
    lib = _lib.load()
    n, q, d, k = tx.size(0), ty.size(0), tx.size(1), int(k)
    with torch.cuda.device(tx.device):
        ws = _matcher_scratch(lib, n, q, k, int(chunk_rows), tx.device)       # (refuses k > _lib.TOPK_MAX_K before anything is allocated)
        values = torch.empty(q, k, dtype=torch.float32, device=tx.device)
        indices = torch.empty(q, k, dtype=torch.int64, device=tx.device)
        _lib.check(lib.hgt_matcher_topk(_ptr(tx), ldx, n, _ptr(ty), ldy, q, d, float(scale), k, int(chunk_rows), _ptr(values), _ptr(indices),
                                        ws.data_ptr(), ws.numel(), _stream(tx)), "hgt_matcher_topk")
    return values, indices


def matcher_rank(tx, ty, index, scale, chunk_rows=0):
    """rank int64 [Q] of candidate index[q] among all N candidates of query q (0 = best; an index outside [0, N) gives -1): the rule is
    np_matcher_rank.  Same tensors and limits as matcher_topk, and the same score bits: matcher_rank(index=indices[:, j]) == j.
    MRR = mean of 1 / (1 + rank), Hits@k = mean of rank < k over the queries with a rank >= 0."""
    tx, ty, ldx, ldy = _matcher_args(tx, ty, "matcher_rank")
    lib = _lib.load()
    n, q, d = tx.size(0), ty.size(0), tx.size(1)
    index = torch.as_tensor(index, device=tx.device).reshape(-1).to(torch.int64).contiguous()
    if index.numel() != q:
        raise ValueError("pyhgt_amd: one index per query")
    with torch.cuda.device(tx.device):
        ws = _matcher_scratch(lib, n, q, 1, int(chunk_rows), tx.device)
        rank = torch.empty(q, dtype=torch.int64, device=tx.device)
        _lib.check(lib.hgt_matcher_rank(_ptr(tx), ldx, n, _ptr(ty), ldy, q, d, float(scale), int(chunk_rows), _ptr(index), _ptr(rank),
                                        ws.data_ptr(), ws.numel(), _stream(tx)), "hgt_matcher_rank")
    return rank
