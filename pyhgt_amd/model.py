"""Host-side mirror of the reference's GNN wrapper ("next" row 1).

`GNN` keeps the constructor, attribute / state_dict names and forward signature of
/root/reference/pyHGT/model.py:54-80: a typed input adapter (`adapt_ws[t]` Linear + tanh, model.py:70-76)
followed by `n_layers` GeneralConv('hgt') layers that all receive the same graph tensors (model.py:78-79).
The adapter runs on the same typed-linear kernels as the layers (no per-type boolean masks, no host sync --
the reference syncs once per type at model.py:73), and one GraphPlan is built for the whole stack.
Inference runs without autograd; with grad enabled the adapter and the layers take their differentiable paths
(pyhgt_amd/autograd.py).  Classifier / Matcher (model.py:3-49) run on the same kernels.
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from . import _lib
from .conv import GeneralConv, GraphPlan, _ptr, _stream
from .metrics import _one_label_form, class_loss, class_predict, matcher_rank, matcher_scale, matcher_topk

__all__ = ["GNN", "Classifier", "Matcher"]


class GNN(nn.Module):
    def __init__(self, in_dim, n_hid, num_types, num_relations, n_heads, n_layers, dropout=0.2, conv_name='hgt',
                 prev_norm=False, last_norm=False, use_RTE=True, deterministic=False, recompute=False):
        super().__init__()
        self.deterministic = bool(deterministic)      # bit-reproducible training (autograd.set_deterministic reaches the layers too)
        self.recompute = bool(recompute)              # memory-lean training of the layers (autograd.set_recompute)
        self.gcs = nn.ModuleList()
        self.num_types = num_types
        self.in_dim = in_dim
        self.n_hid = n_hid
        self.adapt_ws = nn.ModuleList(nn.Linear(in_dim, n_hid) for _ in range(num_types))
        self.drop = nn.Dropout(dropout)
        for _ in range(n_layers - 1):
            self.gcs.append(GeneralConv(conv_name, n_hid, n_hid, num_types, num_relations, n_heads, dropout,
                                        use_norm=prev_norm, use_RTE=use_RTE))
        self.gcs.append(GeneralConv(conv_name, n_hid, n_hid, num_types, num_relations, n_heads, dropout,
                                    use_norm=last_norm, use_RTE=use_RTE))
        self._packed = None
        self._packed_key = None
        if deterministic:
            for gc in self.gcs:
                gc.base_conv.deterministic = True
        if recompute:
            for gc in self.gcs:
                gc.base_conv.recompute = True

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_packed"] = st["_packed_key"] = None
        st.pop("_plist", None)
        st.pop("_tiles", None)
        st.pop("_tiles_key", None)
        return st

    def __setstate__(self, state):
        """Modules pickled by the reference class (torch.save(model), train_paper_field.py:279) lack the cache attributes."""
        super().__setstate__(state)
        self.__dict__.setdefault("_packed", None)
        self.__dict__.setdefault("_packed_key", None)

    def invalidate(self):
        """Forget the packed adapter weights and every layer's packed / prepared images (needed after writes through
        `.data`, which do not bump the parameter versions the caches are keyed on; see HGTConv.invalidate)."""
        self._packed = self._packed_key = None
        self.__dict__.pop("_tiles_key", None)
        self.__dict__.pop("_plist", None)
        for gc in self.gcs:
            if hasattr(gc.base_conv, "invalidate"):
                gc.base_conv.invalidate()

    def _load_from_state_dict(self, *args, **kwargs):
        self._packed = self._packed_key = None
        self.__dict__.pop("_plist", None)
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._packed = self._packed_key = None
        self.__dict__.pop("_plist", None)
        return super()._apply(fn, *args, **kwargs)

    def _pack_adapter(self):
        plist = self.__dict__.get("_plist")
        if plist is None:
            plist = self.__dict__["_plist"] = [p for lin in self.adapt_ws for p in lin.parameters()]
        key = 0                                  # sum of version counters (see HGTConv._pack_parameters)
        for p in plist:
            key += p._version
        if self._packed is None or self._packed_key != key or self.training:
            with torch.no_grad():
                w = torch.stack([lin.weight for lin in self.adapt_ws]).float().contiguous()   # [T, n_hid, in_dim]
                b = torch.stack([lin.bias for lin in self.adapt_ws]).float().contiguous()     # [T, n_hid]
            self._packed, self._packed_key = (w, b), key
        return self._packed

    def _adapter_tiles(self, w, in_dim, n_hid, st, f16=False):
        """Split MFMA tiles of the adapter weights (hgt_split_weights[_f16]), kept until the weights change."""
        key = (w.data_ptr(), self._packed_key, f16)
        if getattr(self, "_tiles_key", None) != key:
            lib = _lib.load()
            nb = C.c_uint64()
            _lib.check(lib.hgt_split_weights_bytes(self.num_types, in_dim, n_hid, C.byref(nb)), "hgt_split_weights_bytes")
            self._tiles = torch.empty(int(nb.value), dtype=torch.uint8, device=w.device)
            _lib.check((lib.hgt_split_weights_f16 if f16 else lib.hgt_split_weights)(_ptr(w), n_hid * in_dim, self.num_types, in_dim, n_hid,
                                                                                      _ptr(self._tiles), st), "hgt_split_weights(adapter)")
            self._tiles_key = key
        return self._tiles

    def forward(self, node_feature, node_type, edge_time, edge_index, edge_type, seeds=None, trim=None):
        """Same argument order as the reference (model.py:69): note edge_time comes third.

        seeds (int64 device tensor of rows, any order, repeats allowed) or trim (a `TrimmedGraph` of `trim_to_seeds` for this graph and
        this many layers): the seed-trimmed forward.  Every layer computes only the rows that can still reach a seed in the layers
        left, and the result is the [len(seeds), n_hid] tensor of the seed rows -- what `forward(...)[seeds]` gives, up to the rounding
        of another kernel route and row grouping.  Dropout masks are drawn over the trimmed rows: another draw than the untrimmed
        step's.  With keep_att, layer l's `.att` is over the edges `trim.edge_order[:trim.n_edges[l]]`."""
        lib = _lib.load()
        if not node_feature.is_cuda:
            raise RuntimeError("pyhgt_amd.GNN runs only on a ROCm GPU tensor; there is no CPU fallback")
        if seeds is not None or trim is not None:
            return self._forward_trimmed(node_feature, node_type, edge_time, edge_index, edge_type, seeds, trim)
        conv0 = self.gcs[0].base_conv
        plan = GraphPlan.cached(node_type, edge_index, edge_type, edge_time if conv0.use_RTE else None,
                                conv0.num_types, conv0.num_relations)
        if self._takes_grad(node_feature):
            h = self._adapt_grad(node_feature, plan)
            for gc in self.gcs:
                h = gc.base_conv(h, node_type, edge_index, edge_type, edge_time, plan=plan)
            return h
        h = self._adapt(node_feature.detach().float().contiguous(), plan)
        for gc in self.gcs:
            h = gc.base_conv(h, node_type, edge_index, edge_type, edge_time, plan=plan)
        return h

    def _takes_grad(self, node_feature):
        return torch.is_grad_enabled() and (node_feature.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _adapt_grad(self, node_feature, plan):
        """The adapter on the rows of `plan`, differentiable: TypedLinearFunction (typed weight gradient
        kernels), then tanh + dropout as in model.py:70-76."""
        from .autograd import TypedLinearFunction, takes_det_route
        rows = plan.row_lists()
        w = torch.stack([lin.weight for lin in self.adapt_ws]).float()
        b = torch.stack([lin.bias for lin in self.adapt_ws]).float()
        h = TypedLinearFunction.apply((rows.rows_all, rows.off_all, plan), self.num_types, self.gcs[0].base_conv.precision,
                                      node_feature.float(), w, b, takes_det_route(self))
        return self.drop(torch.tanh(h))        # rows of a type no adapter claims stay 0 (model.py:70)

    def _adapt(self, x, plan):
        """The adapter on the rows of `plan` without autograd: x float32 [plan.N, in_dim], contiguous -> tanh(adapt_ws[type](x))."""
        lib = _lib.load()
        conv0 = self.gcs[0].base_conv
        rows = plan.row_lists()
        N = x.size(0)
        w, b = self._pack_adapter()
        T, n_hid, in_dim = self.num_types, self.n_hid, self.in_dim
        h = torch.empty(N, n_hid, dtype=torch.float32, device=x.device)
        st = _stream()
        # typed adapter (in_dim is arbitrary, e.g. 129 or 1169): the precision of the layers -- split-bf16 x3 MFMA (its row loader
        # takes any K) or the exact fp32 MFMA kernel
        need_tanh = True
        if conv0.precision in ("bf16x3", "f16x3") and n_hid % 4 == 0:
            f16 = conv0.precision == "f16x3"
            tiles = self._adapter_tiles(w, in_dim, n_hid, st, f16)
            fn = lib.hgt_typed_linear_f16x3 if f16 else lib.hgt_typed_linear_bf16x3
            # adapter + tanh in one kernel where the kernel that takes the shape has the activation epilogue (sampled batches;
            # HGT_ERR_UNSUPPORTED = nothing was launched)
            # (asked for on sampled batches only: with the bit set a large input never takes the x-stationary kernel, which has no
            #  activation epilogue)
            rc = -2 if N >= 65536 else fn(_ptr(x), in_dim, rows.rows_all, rows.off_all, T, N, in_dim, n_hid, _ptr(tiles), _ptr(b), n_hid,
                                          _ptr(h), 0, 0, n_hid, 0, _lib.HGT_LINEAR_TANH, st)
            if rc == 0:
                need_tanh = False
            else:
                _lib.check(fn(_ptr(x), in_dim, rows.rows_all, rows.off_all, T, N, in_dim, n_hid, _ptr(tiles), _ptr(b), n_hid, _ptr(h), 0, 0, n_hid,
                              0, 0, st), "hgt_typed_linear_bf16x3(adapter)")
        else:
            _lib.check(lib.hgt_typed_linear(_ptr(x), in_dim, rows.rows_all, rows.off_all, T, N, in_dim, n_hid, _ptr(w), n_hid * in_dim,
                                            _ptr(b), n_hid, _ptr(h), 0, 0, n_hid, 0, 0, 0, st), "hgt_typed_linear(adapter)")
        # nodes whose type no adapter claims stay zero like the reference's zero-initialised `res` (model.py:70);
        # rows_all[off_all[T] .. off_all[T+1]) are exactly those nodes
        if not (plan.NQ == plan.N and plan.no_unknown_rows):      # (skipped once the plan header says every row has a valid type)
            _lib.check(lib.hgt_zero_rows(rows.rows_all, rows.off_all + 4 * T, n_hid, _ptr(h), st), "hgt_zero_rows")
        if need_tanh:
            _lib.check(lib.hgt_tanh_inplace(_ptr(h), N * n_hid, st), "hgt_tanh_inplace")
        return h

    def _forward_trimmed(self, node_feature, node_type, edge_time, edge_index, edge_type, seeds, trim):
        """forward(..., seeds= / trim=): gather the rows the stack needs, the adapter on them, layer l on the rows and edges of its
        prefix (the rectangular layer: n_q_rows = trim.n_rows[l]), the seed rows of the last layer's output."""
        from .trim import TrimmedGraph, trim_to_seeds
        L = len(self.gcs)
        conv0 = self.gcs[0].base_conv
        if seeds is not None and trim is not None:
            raise ValueError("pyhgt_amd.GNN: pass seeds= or trim=, not both")
        if trim is None:
            trim = trim_to_seeds((node_type, edge_time, edge_index, edge_type), seeds, L, conv0.num_types, conv0.num_relations)
        elif not isinstance(trim, TrimmedGraph):
            raise TypeError("pyhgt_amd.GNN: trim must be a TrimmedGraph (pyhgt_amd.trim_to_seeds)")
        if trim.n_layers != L:
            raise ValueError("pyhgt_amd.GNN: the trim was built for %d layers, this stack has %d" % (trim.n_layers, L))
        if trim.n_nodes != node_feature.size(0):
            raise ValueError("pyhgt_amd.GNN: the trim was built for a graph of %d nodes, node_feature has %d rows"
                             % (trim.n_nodes, node_feature.size(0)))
        if trim.num_types is None:
            trim.num_types, trim.num_relations = conv0.num_types, conv0.num_relations
        if conv0.use_RTE and trim.edge_time is None:
            raise ValueError("use_RTE=True needs edge_time (conv.py:91-92)")
        grad = self._takes_grad(node_feature)
        n0, S = trim.n_rows[0], trim.n_seeds
        if n0 == 0:                                  # no seed: no row, no layer
            return torch.zeros(S, self.n_hid, dtype=torch.float32, device=node_feature.device)
        lib = _lib.load()
        if grad:
            h = self._adapt_grad(node_feature if trim.gathered else node_feature[trim.order], trim.plan(1, conv0.use_RTE))
        elif trim.gathered:                          # (a NeighbourhoodGraph: the rows are the trim's already, n_nodes = n_rows[0])
            h = self._adapt(node_feature.detach().float().contiguous(), trim.plan(1, conv0.use_RTE))
        else:
            x = node_feature.detach().float()
            x = x if x.stride(1) == 1 else x.contiguous()
            xs = torch.empty(n0, self.in_dim, dtype=torch.float32, device=x.device)
            _lib.check(lib.hgt_gather_rows(_ptr(x), x.stride(0), _ptr(trim.order32), n0, self.in_dim, _ptr(xs), _stream()),
                       "hgt_gather_rows(trim)")
            h = self._adapt(xs, trim.plan(1, conv0.use_RTE))
        for l, gc in enumerate(self.gcs, start=1):
            nt, ei, et, tm = trim.layer_graph(l)
            h = gc.base_conv(h, nt, ei, et, tm, plan=trim.plan(l, gc.base_conv.use_RTE), n_q_rows=trim.n_rows[l])
        if grad:
            return h[trim.out_rows]
        out = torch.empty(S, self.n_hid, dtype=torch.float32, device=h.device)
        _lib.check(lib.hgt_gather_rows(_ptr(h), h.stride(0), _ptr(trim.out_rows32), S, self.n_hid, _ptr(out), _stream()),
                   "hgt_gather_rows(seeds)")
        return out


def _det(module):
    from .autograd import takes_det_route      # (lazily, like GNN.forward: autograd imports conv, not model)
    return takes_det_route(module)


def _dense_linear(x, weight, bias, scale=1.0, deterministic=False):
    """y = (x @ weight^T + bias) * scale on the exact fp32 MFMA typed-linear kernel (one group = every row)."""
    lib = _lib.load()
    if not x.is_cuda:
        raise RuntimeError("pyhgt_amd heads run only on a ROCm GPU tensor; there is no CPU fallback")
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        # differentiable path: same kernel forward, typed weight-gradient kernels backward (pyhgt_amd/autograd.py)
        from .autograd import TypedLinearFunction
        xx = x.float().contiguous()
        n = xx.size(0)
        rows = torch.arange(n, dtype=torch.int32, device=x.device)
        off = torch.tensor([0, n], dtype=torch.int32, device=x.device)
        w = (weight.float() * scale).unsqueeze(0)
        b = (bias.float() * scale).unsqueeze(0) if bias is not None else None
        return TypedLinearFunction.apply((rows.data_ptr(), off.data_ptr(), (rows, off)), 1, "fp32", xx, w, b, deterministic)
    x = x.detach().float().contiguous()
    n, k = x.shape
    n_out = weight.size(0)
    w = (weight.detach().float() * scale).contiguous()
    b = (bias.detach().float() * scale).contiguous() if bias is not None else None
    rows = torch.arange(n, dtype=torch.int32, device=x.device)
    off = torch.tensor([0, n], dtype=torch.int32, device=x.device)
    y = torch.empty(n, n_out, dtype=torch.float32, device=x.device)
    _lib.check(lib.hgt_typed_linear(_ptr(x), k, _ptr(rows), _ptr(off), 1, n, k, n_out, _ptr(w), 0, _ptr(b), 0, _ptr(y), 0, 0, n_out,
                                    0, 0, 0, _stream()), "hgt_typed_linear(head)")
    return y


class Classifier(nn.Module):
    """model.py:3-14: log_softmax(linear(x).squeeze(), dim=-1) on the seed rows."""

    def __init__(self, n_hid, n_out, deterministic=False):
        super().__init__()
        self.deterministic = bool(deterministic)
        self.n_hid, self.n_out = n_hid, n_out
        self.linear = nn.Linear(n_hid, n_out)

    def forward(self, x):
        tx = _dense_linear(x.reshape(-1, self.n_hid), self.linear.weight, self.linear.bias, deterministic=_det(self))
        if tx.requires_grad:
            return torch.log_softmax(tx, dim=-1).reshape(*x.shape[:-1], self.n_out).squeeze()      # model.py:11, under autograd
        out = torch.empty_like(tx)
        _lib.check(_lib.load().hgt_log_softmax_rows(_ptr(tx), tx.size(0), tx.size(1), _ptr(out), _stream()), "hgt_log_softmax_rows")
        return out.reshape(*x.shape[:-1], self.n_out).squeeze()

    def loss(self, x, labels=None, index=None, columns=None, count=None, reduce="mean"):
        """The training loss of the scripts on the seed rows x [n, n_hid] without the [n, n_out] log-probabilities: the linear layer
        (differentiable, honours `deterministic`), then metrics.class_loss on its raw logits -- NLLLoss() with `index`
        (train_paper_venue.py:86), KLDivLoss('batchmean') with `labels` or `columns` / `count` (train_paper_field.py:87)."""
        _one_label_form(labels, index, columns, count)
        tx = _dense_linear(x.reshape(-1, self.n_hid), self.linear.weight, self.linear.bias, deterministic=_det(self))
        return class_loss(tx, labels=labels, index=index, columns=columns, count=count, reduce=reduce)

    def logits(self, x, what="logits", rule="torch.nn.functional.linear"):
        """the raw logits [n, n_out] of the linear layer on rows x [n, n_hid], without a graph: what predict and vote work on"""
        if not x.is_cuda:
            raise RuntimeError("pyhgt_amd: Classifier.%s runs only on a ROCm GPU tensor; %s is the definition on the host" % (what, rule))
        with torch.no_grad():
            return _dense_linear(x.reshape(-1, self.n_hid), self.linear.weight, self.linear.bias, deterministic=_det(self))

    def predict(self, x, **kw):
        """The predictions of the rows x [n, n_hid] and, with labels, the per-split accuracy counts of train_ogbn_mag.py:165-191: the
        linear layer, then metrics.class_predict(logits, **kw) on its raw logits -- no [n, n_out] log-probabilities.  Not differentiable."""
        return class_predict(self.logits(x, "predict", "np_class_predict"), **kw)

    def vote(self, x, table, ids, piece_sizes=None):
        """One sampled sub-graph's (or one stack's) share of a voted evaluation (eval_ogbn_mag.py:148-150): the linear layer, then
        table.add(logits, ids, piece_sizes) -- the log-softmax is formed inside the add, no [n, n_out] log-probabilities."""
        return table.add(self.logits(x, "vote", "np_vote_add"), ids, piece_sizes)

    def __repr__(self):
        return '{}(n_hid={}, n_out={})'.format(self.__class__.__name__, self.n_hid, self.n_out)


class Matcher(nn.Module):
    """model.py:16-49: scaled dot product between projected node pairs (link prediction), with the reference's
    inference-time cache of the projected candidates."""

    def __init__(self, n_hid, deterministic=False):
        super().__init__()
        self.deterministic = bool(deterministic)
        self.left_linear = nn.Linear(n_hid, n_hid)
        self.right_linear = nn.Linear(n_hid, n_hid)
        self.sqrt_hd = math.sqrt(n_hid)
        self.n_hid = n_hid
        self.cache = None

    def forward(self, x, y, infer=False, pair=False):
        ty = _dense_linear(y, self.right_linear.weight, self.right_linear.bias, deterministic=_det(self))
        if infer and self.cache is not None:
            tx = self.cache
        else:
            tx = _dense_linear(x, self.left_linear.weight, self.left_linear.bias, deterministic=_det(self))
            if infer:
                self.cache = tx
        if pair and (tx.requires_grad or ty.requires_grad):
            return (tx * ty).sum(dim=-1) / self.sqrt_hd                                            # model.py:41,44, under autograd
        if pair:
            out = torch.empty(tx.size(0), dtype=torch.float32, device=tx.device)
            _lib.check(_lib.load().hgt_row_dot(_ptr(tx), _ptr(ty), tx.size(0), self.n_hid, 1.0 / self.sqrt_hd, _ptr(out), _stream()),
                       "hgt_row_dot")
            return out
        # tx @ ty^T / sqrt(n_hid): the typed-linear kernel with ty as the "weight" and no bias
        return _dense_linear(tx, ty / self.sqrt_hd, None, deterministic=_det(self))

    def _projected(self, x, y, infer, what):
        """(tx, ty) of forward(): candidates x through left_linear -- under infer=True from / into self.cache --, queries y through
        right_linear; without autograd"""
        if not y.is_cuda or not ((infer and self.cache is not None) or x.is_cuda):
            raise RuntimeError("pyhgt_amd: Matcher.%s runs only on ROCm GPU tensors; metrics.np_matcher_%s is the definition on the host"
                               % (what, "topk" if what == "topk" else "rank"))
        with torch.no_grad():
            ty = _dense_linear(y, self.right_linear.weight, self.right_linear.bias, deterministic=_det(self))
            if infer and self.cache is not None:
                tx = self.cache
            else:
                tx = _dense_linear(x, self.left_linear.weight, self.left_linear.bias, deterministic=_det(self))
                if infer:
                    self.cache = tx
        return tx.detach(), ty

    def topk(self, x, y, k, infer=False):
        """(values float32 [Q, k], indices int64 [Q, k]): for every query row of y the k candidates (rows of x) the model scores highest,
        best first, over ALL candidates and without the [N, Q] matrix of forward(x, y, infer=True) -- one streaming pass over the
        projected candidates (metrics.matcher_topk; the rule is metrics.np_matcher_topk: ties go to the lower row, a NaN stands above
        +inf, slots beyond N hold -inf / -1).  The score is (left_linear(x) . right_linear(y)) * fl32(1 / sqrt(n_hid)).  infer=True uses
        and fills self.cache exactly as forward does.  Not differentiable; 1 <= k <= 128 (_lib.TOPK_MAX_K), n_hid % 4 == 0, <= 1024."""
        tx, ty = self._projected(x, y, infer, "topk")
        return matcher_topk(tx, ty, k, matcher_scale(self.n_hid))

    def rank_of(self, x, y, index, infer=False):
        """rank int64 [Q]: how many of ALL candidates (rows of x) the model places before candidate index[q] for query row q of y --
        0 = the model's first answer, -1 for an index outside [0, N) (metrics.matcher_rank; the rule is metrics.np_matcher_rank).  The
        scores are topk's bit for bit, so rank_of(x, y, indices[:, j]) == j.  The metrics of a link-prediction evaluation follow from the
        ranks: MRR = mean of 1 / (1 + rank), Hits@k = mean of rank < k.  infer=True as in forward.  Not differentiable."""
        tx, ty = self._projected(x, y, infer, "rank_of")
        return matcher_rank(tx, ty, index, matcher_scale(self.n_hid))

    def __repr__(self):
        return '{}(n_hid={})'.format(self.__class__.__name__, self.n_hid)
