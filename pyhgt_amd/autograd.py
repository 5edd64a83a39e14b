"""Training path of HGTConv / DenseHGTConv: forward that keeps its intermediates + the hand-written backward.

The reference trains through autograd over conv.py:60-134 (`loss.backward()`, OAG/train_paper_field.py:249,
ogbn-mag/train_ogbn_mag.py:172).  Here a `torch.autograd.Function` wraps the HIP kernels: the forward is the same
node-level algebra as the inference path (typed Q|K|V projections once per node, target-side relation transforms, softmax
over in-edges, relation-wise aggregation on the matrix cores), run kernel by kernel so that Q, K, V, the attention weights,
the aggregate and the a_linear output stay available; the backward strings together the kernels of
csrc/hgt_bwd_*.hip + the forward kernels on the transposed graph (the derivation is in the header of csrc/hgt_bwd_update.hip).

Layout of this file: TENSOR_SLOTS (the one statement of the Function's input order), the kernel-choice predicates, the typed-linear
route (_typed_linear / _wgrad, shared with TypedLinearFunction), _Step (the per-call context: kernel wrappers, then the named steps
of the forward and of the backward, named after the steps of csrc/hgt_api.hip where they correspond), and the two Functions, whose
forward / backward only dispatch to the steps.

PyTorch's role: the Function boundary, parameter packing with differentiable stack/cat/pad ops (so the gradients of the
packed arrays flow back to the reference-named parameters by themselves), tiny O(R H d_k^2) / O(T 240 d) chain-rule steps on
relation matrices and temporal tables, and the dropout mask (torch RNG, like the reference's nn.Dropout at conv.py:125).
There is no CPU or eager fallback: CPU tensors raise.
"""
import ctypes as C
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import check
from .conv import _ptr, _stream

__all__ = ["hgt_conv_train", "training_supported", "logits_form", "outer_form", "spmm_takes_items", "takes_det_route", "set_deterministic",
           "takes_recompute", "set_recompute", "TypedLinearFunction", "MAX_TRAIN_DK_PAD"]


MAX_TRAIN_DK_PAD = 256      # widest (padded) head the training path covers: the matrix-core form of hgt_edge_spmm ends there

# Inputs of _HGTConvTrain: PLAIN_SLOTS (no gradient), then these tensors under the names of HGTConv._pack_parameters (None where a
# layer has no such parameter).  hgt_conv_train builds .apply's arguments from this table, forward reads them by name and backward
# returns its gradients through it: a new parameter is added HERE and in the step that uses it.
PLAIN_SLOTS = ("layer", "plan", "drop_masks")
TENSOR_SLOTS = ("x", "w_qkv", "b_qkv", "w_a", "b_a", "ratt", "rmsg", "rpri", "skip", "ln_w", "ln_b", "rte_emb", "rte_w", "rte_b",
                "mid_w", "mid_b", "out_w", "out_b", "out_ln_w", "out_ln_b")
_SPLIT = ("bf16x3", "f16x3")      # precisions of the split-bf16 x3 MFMA GEMMs (the differentiable path evaluates "f16x3" layers with the bf16 split)


def training_supported(out_dim, n_heads):
    """(ok, reason): can a layer of this width / head count run the training forward + backward?  Host-only (the layout
    arithmetic of hgt_layout_for); the one statement of the limit -- hgt_conv_train's guard and the tests both call it.
    Heads of up to 64 padded columns take hgt_relation_outer, 128 and 256 hgt_relation_outer_wide; wider heads (out_dim 512
    with one head, 1024 with two) run inference only."""
    lay = _lib.layout_for(out_dim, n_heads)
    if lay.dk_pad > MAX_TRAIN_DK_PAD:
        return False, ("the backward pass supports heads of at most %d (padded) columns; out_dim=%d / n_heads=%d gives %d.  "
                       "Inference has no such limit (INTEGRATION.md, training limits)" % (MAX_TRAIN_DK_PAD, out_dim, n_heads, lay.dk_pad))
    return True, ""


# -- which kernel runs (host predicates; the tests call them to aim their cases at each branch) -----------------------------------
def logits_form(dk_pad):
    """'mfma' (hgt_edge_logits_mfma) or 'valu' (hgt_edge_logits).  Wide heads: the vector-ALU kernel cannot hold a head's relation
    matrix in registers and re-reads it per edge (604 ms per call at 1 M nodes / 10 M edges, n_hid 768 / 8 heads) -- the matrix-core
    form of the inference path instead (18 ms; 3-term split products like the aggregation's, also for precision='fp32' layers)."""
    return "mfma" if dk_pad >= 128 else "valu"


def outer_form(dk_pad):
    """Entry point of the relation outer products.  Heads of up to 64 padded columns: register-resident blocks per wavefront;
    128 / 256: one workgroup per 128 x 128 block."""
    return "hgt_relation_outer" if dk_pad <= 64 else "hgt_relation_outer_wide"


def spmm_takes_items(N, E, R, ld_out, out_col):
    """Does a gather pass take hgt_edge_spmm_items (else hgt_edge_spmm)?  Sampled batches: the item-parallel form (one wavefront
    per <= 16-edge item + an ordered merge) -- the sub-tile kernel's wavefronts each walk sixteen targets' edges one after the other
    (285 vs ~25 us per call at c3).  The kernel stores 4-column vectors and keeps a relation per lane."""
    return N < 65536 and E > 0 and R < 64 and ld_out % 4 == 0 and out_col % 4 == 0


def takes_det_route(module):
    """Does `module` (HGTConv, DenseHGTConv, GNN, Classifier, Matcher) train on the atomic-free `_det` entry points?  The one
    predicate: its `deterministic` attribute and nothing else -- in particular not torch.use_deterministic_algorithms, which callers
    switch on around unrelated code (a module unpickled without the attribute is a default one)."""
    return bool(getattr(module, "deterministic", False))


def set_deterministic(module, on=True):
    """Set `deterministic` on every pyhgt_amd module of a model (the layers, GNN, Classifier, Matcher).  On a model built by the
    reference's own GNN after install_into (whose constructor cannot pass the keyword) that is the layers: the reference's adapter and
    heads are torch modules this switch does not reach.  Returns the module.  With it, a training
    step executes no floating-point atomic and sums every reduction in an order fixed by the problem sizes: the same build, device
    model, inputs and seed give the same bits (reproducible training)."""
    from .conv import HGTConv
    from .model import GNN, Classifier, Matcher
    for m in module.modules():
        if isinstance(m, (HGTConv, GNN, Classifier, Matcher)):
            m.deterministic = bool(on)
    return module


def takes_recompute(module):
    """Does `module` train in the memory-lean mode (its `recompute` attribute and nothing else; a module unpickled without the
    attribute is a default one)?  Only the layers act on it: the adapter and the heads keep nothing that could be recomputed."""
    return bool(getattr(module, "recompute", False))


def set_recompute(module, on=True):
    """Set `recompute` on every pyhgt_amd module of a model (the layers, GNN, Classifier, Matcher), like set_deterministic.  Returns
    the module.  With it a layer's training forward keeps neither Q|K|V, the a_linear output (HGTConv) nor its dropout masks between
    forward and backward: the backward projects Q|K|V again, runs a_linear again and writes the masks again from the layer call's
    seed (hgt_dropout_mask) -- the same kernels on the same inputs, hence the same bits as the tensors the default mode keeps
    (memory-lean training).  The masks themselves come from the counter-based generator of csrc/hgt_dropout.hip
    instead of torch.bernoulli: a seeded run repeats, but draws other masks than the default mode does."""
    from .conv import HGTConv
    from .model import GNN, Classifier, Matcher
    for m in module.modules():
        if isinstance(m, (HGTConv, GNN, Classifier, Matcher)):
            m.recompute = bool(on)
    return module


# Dropout of the recompute mode.  One 64-bit seed per layer call; dropout site s of the call (0: the a_linear output, conv.py:125 /
# 261; 1: DenseHGTConv's out_linear output, conv.py:273) is hgt_dropout_apply / hgt_dropout_mask at (seed, s << DROP_SITE_SHIFT, keep):
# a site covers at most 2^31 elements = 2^29 counter values, so the counter ranges of two sites never meet.
DROP_SITE_SHIFT = 40
_DropSite = namedtuple("_DropSite", "seed offset keep")


class _CounterDropout(namedtuple("_CounterDropout", "seed keep offsets")):
    """(seed, keep, offsets): what a layer call in recompute mode keeps of its dropout, and `layer.last_dropout_state`."""

    def site(self, s):
        return _DropSite(self.seed, self.offsets[s], self.keep) if s < len(self.offsets) else None


def _det_ws(dev, name, *size_args):
    """(pointer, bytes, tensor) of the workspace of a `_det` entry point: sized by its `<name>_bytes` host function; the caching
    allocator hands the block to the next call when the tensor dies (stream-ordered: one workspace is live at a time)."""
    nb = C.c_uint64()
    check(getattr(_lib.load(), name + "_bytes")(*size_args, C.byref(nb)), name + "_bytes")
    t = torch.empty(max(int(nb.value), 16), dtype=torch.uint8, device=dev)
    return t.data_ptr(), int(nb.value), t


def _reduce_call(det, dev, name, size_args, *args, det_name=None):
    """A backward step with a reduction: `name`(*args, stream) on the atomic route; on the det route `name`_det (or det_name) with the
    same leading arguments + the workspace that `..._det_bytes`(*size_args) asks for.  The outputs follow _reduce_out."""
    if det:
        det_name = det_name or name + "_det"
        wp, wb, keep = _det_ws(dev, det_name, *size_args)
        check(getattr(_lib.load(), det_name)(*args, wp, wb, _stream()), det_name)
    else:
        check(getattr(_lib.load(), name)(*args, _stream()), name)


def _reduce_out(det, dev, *shape):
    """Output of a _reduce_call: the atomic route accumulates into a zeroed tensor, the det route overwrites an empty one."""
    return (torch.empty if det else torch.zeros)(*shape, dtype=torch.float32, device=dev)


# -- the typed-linear route: the layer's GEMMs and TypedLinearFunction ---------------------------------------------------------
def _typed_linear(split, x, ldx, rows, off, n_groups, n_rows, k, n_out, W, w_off, wgs, bias, b_off, bgs, outs, block_cols, by_pos=0,
                  prologue=0):
    """y = prologue(x[rows]) W[g]^T + b[g]; W / bias given as (tensor, element offset).  outs: up to 3 column blocks of block_cols.
    split: the split-bf16 x3 MFMA kernel (where its 4-column stores fit) instead of the exact fp32 one."""
    lib = _lib.load()
    o = [_ptr(t) for t in outs] + [0] * (3 - len(outs))
    wp = W.data_ptr() + 4 * w_off
    bp = 0 if bias is None else bias.data_ptr() + 4 * b_off
    if split and n_out % 4 == 0 and block_cols % 4 == 0:
        nb = C.c_uint64()
        check(lib.hgt_split_weights_bytes(n_groups, k, n_out, C.byref(nb)), "hgt_split_weights_bytes")
        tiles = torch.empty(int(nb.value), dtype=torch.uint8, device=x.device)
        check(lib.hgt_split_weights(wp, wgs, n_groups, k, n_out, _ptr(tiles), _stream()), "hgt_split_weights")
        check(lib.hgt_typed_linear_bf16x3(_ptr(x), ldx, rows, off, n_groups, n_rows, k, n_out, _ptr(tiles), bp, bgs, o[0], o[1], o[2],
                                          block_cols, by_pos, prologue, _stream()), "hgt_typed_linear_bf16x3")
        tiles.record_stream(torch.cuda.current_stream())
    else:
        check(lib.hgt_typed_linear(_ptr(x), ldx, rows, off, n_groups, n_rows, k, n_out, wp, wgs, bp, bgs, o[0], o[1], o[2], block_cols,
                                   by_pos, prologue, 0, _stream()), "hgt_typed_linear")


def _wgrad(split, A, lda, B, ldb, rows, off, n_groups, n_rows, m, n_cols, with_colsum=True, det=False):
    """(dW[g] = A_g^T B_g, db[g] = column sums of A_g or None): split-bf16 x3 MFMA kernel (both from one pass) for split precisions,
    the exact fp32 MFMA kernel + the column-sum kernel otherwise.  det: the same kernels' atomic-free forms (partials per row chunk,
    summed in chunk order)."""
    dev, sizes = A.device, (n_groups, n_rows, m, n_cols)
    dw = _reduce_out(det, dev, n_groups, m, n_cols)
    db = _reduce_out(det, dev, n_groups, m) if with_colsum else None
    wgrad_args = (_ptr(A), lda, _ptr(B), ldb, rows, off, n_groups, n_rows, m, n_cols, _ptr(dw), m * n_cols)
    if split:
        _reduce_call(det, dev, "hgt_typed_wgrad_bf16x3", sizes, *wgrad_args, _ptr(db), m)
    else:
        _reduce_call(det, dev, "hgt_typed_wgrad", sizes, *wgrad_args)
        if with_colsum:
            _reduce_call(det, dev, "hgt_typed_colsum", sizes[:3], _ptr(A), lda, rows, off, n_groups, n_rows, m, _ptr(db), m)
    return dw, db


# -- saved state by name ------------------------------------------------------------------------------------------------------
def _save_named(ctx, tensors):
    """Save {name: tensor or None} for the backward: the tensors through ctx.save_for_backward (torch keeps its version-counter
    checks and the graph's lifetime rules), the names on the side."""
    ctx.saved_names = tuple(k for k, t in tensors.items() if t is not None)
    ctx.absent_names = tuple(k for k, t in tensors.items() if t is None)
    ctx.save_for_backward(*(tensors[k] for k in ctx.saved_names))


def _load_named(ctx):
    """What _save_named kept, as a namespace; a tensor that was absent is None."""
    return SimpleNamespace(**dict.fromkeys(ctx.absent_names), **dict(zip(ctx.saved_names, ctx.saved_tensors)))


def _rte_row_lists(T, dev):
    rows = (torch.arange(T * _lib.HGT_RTE_LEN, device=dev) % _lib.HGT_RTE_LEN).to(torch.int32)
    off = (torch.arange(T + 1, device=dev) * _lib.HGT_RTE_LEN).to(torch.int32)
    return rows, off


class _Step:
    """One forward or backward call of a layer on a plan: sizes, the kernel wrappers (all on the current stream), then the named
    steps.  p = the Function's tensor inputs by name, s = the saved tensors by name."""

    def __init__(self, layer, plan, lay):
        self.lib = _lib.load()
        self.layer, self.plan, self.lay = layer, plan, lay
        self.T, self.R, self.Hreal = layer.num_types, layer.num_relations, layer.n_heads
        self.H = lay.heads                                   # kernels run with the layout's head count (extra heads: zero)
        self.dk, self.dkp, self.dp = lay.d_k, lay.dk_pad, lay.d_pad
        self.din, self.dout = layer.in_dim, layer.out_dim
        # data gradients (d gelu(agg), dx) run on the layer's own typed-linear kernels: split-bf16 x3 for split precisions, relative
        # error ~1e-5, two orders below the gradient tolerance; precision='fp32' layers keep the exact typed-linear kernel.  The
        # relation transforms of every hgt_edge_spmm -- the training forward's aggregation included -- are ALWAYS split-bf16 MFMA
        # products under grad, also for precision='fp32': ~1e-5 away from the exact VALU aggregation of the inference path
        self.split = layer.precision in _SPLIT
        self.det = takes_det_route(layer)                    # every atomic site of the step takes its `_det` entry point
        self.use_norm = bool(layer.use_norm)
        # N nodes carry K / V; the first NQ of them are the targets (they alone carry Q, an aggregate, an update and an output row).
        # NQ < N: a rank of a destination partition, whose rows [NQ, N) are source-only halo rows (pyhgt_amd/dist.py)
        self.N, self.NQ, self.E = plan.N, plan.NQ, plan.E
        self.dev = plan.device
        self.rows = plan.row_lists()
        self.halo = plan.halo_row_lists() if self.NQ < self.N else None      # (rows, offsets, count): the typed list of rows [NQ, N)
        self._scratch = {}

    def new(self, *shape, zero=False, dtype=torch.float32):
        return (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=self.dev)

    def graph(self, plan):
        """Leading arguments of every edge kernel."""
        return plan.ptr, plan.N, plan.E, self.T, self.R, self.H

    def node_linear(self, x, k, n_out, W, wgs, bias, bgs, out, prologue=0):
        """out = prologue(x) W[type]^T + b[type] over the target rows of a known type (the others stay unwritten)."""
        _typed_linear(self.split, x, k, self.rows.rows_q, self.rows.off_q, self.T, self.NQ, k, n_out, W, 0, wgs, bias, 0, bgs, [out], n_out,
                      prologue=prologue)

    # -- relation matrices ------------------------------------------------------------------------------------
    def pack(self, att_like, msg_like, pri):
        """hgt_relation_pack: (att_t[r,h,c,k] = att_like[r,h,k,c] * pri / sqrt(dk), msg_p = msg_like), zero padded to dk_pad."""
        R, H, dkp = self.R, self.H, self.dkp
        att_t, msg_p = self.new(R, H, dkp, dkp), self.new(R, H, dkp, dkp)
        check(self.lib.hgt_relation_pack(_ptr(att_like.contiguous()), _ptr(msg_like.contiguous()), _ptr(pri.contiguous()), R, self.Hreal, H,
                                         self.dk, dkp, _ptr(att_t), _ptr(msg_p), _stream()), "hgt_relation_pack")
        return att_t, msg_p

    def frags(self, msg_p):
        nb = C.c_uint64()
        check(self.lib.hgt_relation_frag_bytes(self.R, self.H, self.dkp, C.byref(nb)), "hgt_relation_frag_bytes")
        if nb.value == 0:
            raise RuntimeError("pyhgt_amd: training needs a layout the matrix-core aggregation covers: heads of at most %d (padded) "
                               "columns, this layout has %d (autograd.training_supported)" % (MAX_TRAIN_DK_PAD, self.dkp))
        f = self.new(int(nb.value), dtype=torch.uint8)
        check(self.lib.hgt_relation_frag_pack(_ptr(msg_p), self.R, self.H, self.dkp, _ptr(f), _stream()), "hgt_relation_frag_pack")
        return f

    # -- edge phase -------------------------------------------------------------------------------------------
    def logits(self, plan, Q, K, rte_k, att_t):
        out = self.new(plan.E, self.H)
        if logits_form(self.dkp) == "mfma":
            frag = self.frags(att_t)
            check(self.lib.hgt_edge_logits_mfma(*self.graph(plan), self.dkp, _ptr(Q), _ptr(K), _ptr(rte_k), _ptr(att_t), _ptr(frag), 0,
                                                _ptr(out), _stream()), "hgt_edge_logits_mfma")
            frag.record_stream(torch.cuda.current_stream())
        else:
            check(self.lib.hgt_edge_logits(*self.graph(plan), self.dkp, _ptr(Q), _ptr(K), _ptr(rte_k), _ptr(att_t), _ptr(out), _stream()),
                  "hgt_edge_logits")
        return out

    def _items_scratch(self, plan):
        """Scratch of the item-parallel gather passes (sampled batches), one buffer per plan size, reused by every pass of this call."""
        key = ("items", plan.E)
        buf = self._scratch.get(key)
        if buf is None:
            nb = C.c_uint64()
            check(self.lib.hgt_edge_aggregate_items_bytes(plan.E, self.H, self.dkp, C.byref(nb)), "hgt_edge_aggregate_items_bytes")
            buf = self._scratch[key] = self.new(max(int(nb.value), 16), dtype=torch.uint8)
        return buf

    def spmm(self, plan, w, rows_ptr, rte_rows, f_p, f_frag, out, out_col, ld_out, n_q_rows):
        """out[:, out_col : out_col + dp] = sum_r (sum_e w_e rows[src_e]) F_r over the in-edges of every target of `plan`."""
        optr = out.data_ptr() + 4 * out_col
        if spmm_takes_items(plan.N, plan.E, self.R, ld_out, out_col):
            sc = self._items_scratch(plan)
            rc = self.lib.hgt_edge_spmm_items(*self.graph(plan), self.dkp, _ptr(w), rows_ptr, _ptr(rte_rows), _ptr(f_frag), optr, ld_out,
                                              n_q_rows, _ptr(sc), sc.numel(), _stream())
            if rc == 0:
                sc.record_stream(torch.cuda.current_stream())
                return
            if rc != -2:      # HGT_ERR_UNSUPPORTED = nothing was launched: the sub-tile kernel below takes the pass
                check(rc, "hgt_edge_spmm_items")
        if self.det:      # hub targets: one partial per piece, summed in piece order
            hp, hb, hub = _det_ws(self.dev, "hgt_edge_spmm_det", plan.E, self.H, self.dkp, self.R)
            check(self.lib.hgt_edge_spmm_det(*self.graph(plan), self.dkp, _ptr(w), rows_ptr, _ptr(rte_rows), _ptr(f_p), _ptr(f_frag), optr,
                                             ld_out, n_q_rows, hp, hb, _stream()), "hgt_edge_spmm_det")
            return
        nb = C.c_uint64()
        check(self.lib.hgt_hub_workspace_bytes(plan.E, self.H, self.dkp, C.byref(nb)), "hgt_hub_workspace_bytes")
        hub = self.new(max(int(nb.value), 256), dtype=torch.uint8)
        check(self.lib.hgt_edge_spmm(*self.graph(plan), self.dkp, _ptr(w), rows_ptr, _ptr(rte_rows), _ptr(f_p), _ptr(f_frag), optr, ld_out,
                                     n_q_rows, _ptr(hub), _stream()), "hgt_edge_spmm")
        hub.record_stream(torch.cuda.current_stream())

    def to_edge_ids(self, plan, sorted_vals, out_heads=None):
        """Per-edge values in plan order -> the caller's edge order.  out_heads: row stride of the result (the layout's head count;
        self.att wants the model's)."""
        out = torch.empty_like(sorted_vals) if out_heads is None else self.new(plan.E, out_heads)
        check(self.lib.hgt_att_export(*self.graph(plan), _ptr(sorted_vals), _ptr(out), out.size(1), _stream()), "hgt_att_export")
        return out

    def to_sorted(self, plan, by_id):
        out = torch.empty_like(by_id)
        check(self.lib.hgt_edge_gather_sorted(*self.graph(plan), _ptr(by_id), _ptr(out), _stream()), "hgt_edge_gather_sorted")
        return out

    def outer(self, plan, w, a, rte_a, b):
        """out[r][h] = sum over the edges of relation r of w_e a[src_e][h]^T b[dst_e][h]  (det: partials per slice of the plan's item
        list, summed in slice order)."""
        out = _reduce_out(self.det, self.dev, self.R, self.H, self.dkp, self.dkp)
        _reduce_call(self.det, self.dev, outer_form(self.dkp), (plan.N, plan.E, self.T, self.R, self.H, self.dkp), *self.graph(plan), self.dkp,
                     _ptr(w), _ptr(a), _ptr(rte_a), _ptr(b), _ptr(out))
        return out

    def drop_(self, t, mask):
        """t *= mask: a float mask tensor, or a _DropSite of the recompute mode (the mask is generated on the fly)."""
        if isinstance(mask, _DropSite):
            check(self.lib.hgt_dropout_apply(_ptr(t), t.numel(), mask.seed, mask.offset, mask.keep, _stream()), "hgt_dropout_apply")
        elif mask is not None:
            check(self.lib.hgt_mul_inplace(_ptr(t), _ptr(mask), t.numel(), _stream()), "hgt_mul_inplace")

    def drop_mask(self, site):
        """The [NQ, out_dim] float mask drop_ applied at `site` (None: no dropout), written again for the backward kernels."""
        if site is None:
            return None
        m = self.new(self.NQ, self.dout)
        check(self.lib.hgt_dropout_mask(_ptr(m), m.numel(), site.seed, site.offset, site.keep, _stream()), "hgt_dropout_mask")
        return m

    def node_update_bwd(self, *args):
        """hgt_node_update_bwd_ex(*args, stream), or its atomic-free form (one partial per wavefront's row range, summed in range order)."""
        _reduce_call(self.det, self.dev, "hgt_node_update_bwd_ex", (self.NQ, self.dout, self.T), *args, det_name="hgt_node_update_bwd_det")

    # == forward steps (the message path, conv.py:60-111, is shared by both layers) ==========================================
    def relation_images(self, p):
        att_t, msg_p = self.pack(p.ratt, p.rmsg, p.rpri)
        return att_t, msg_p, self.frags(msg_p)

    def project(self, x, p):
        """Q|K|V once per node (conv.py:96-97,103), as one array [Q: NQ rows; K: N rows; V: N rows] (qkv_views).  Source-only rows
        get K|V alone: the 2 dp weight rows behind Q's, over the typed list of the rows [NQ, N)."""
        dp, din, N, NQ = self.dp, self.din, self.N, self.NQ
        qkv = self.new(NQ + 2 * N, dp)
        Q, K, V = self.qkv_views(qkv)
        if NQ == N:
            _typed_linear(self.split, x, din, self.rows.rows_all, self.rows.off_all, self.T, N, din, 3 * dp, p.w_qkv, 0, 3 * dp * din,
                          p.b_qkv, 0, 3 * dp, [Q, K, V], dp)
            return qkv
        _typed_linear(self.split, x, din, self.rows.rows_q, self.rows.off_q, self.T, NQ, din, 3 * dp, p.w_qkv, 0, 3 * dp * din,
                      p.b_qkv, 0, 3 * dp, [Q, K, V], dp)
        h_rows, h_off, n_h = self.halo
        if n_h:
            _typed_linear(self.split, x, din, h_rows.data_ptr(), h_off.data_ptr(), self.T, n_h, din, 2 * dp, p.w_qkv, dp * din, 3 * dp * din,
                          p.b_qkv, dp, 3 * dp, [K, V], dp)
        return qkv

    def qkv_views(self, qkv):
        """(Q [NQ, dp], K [N, dp], V [N, dp]) of project's array."""
        N, NQ = self.N, self.NQ
        return qkv[:NQ], qkv[NQ:NQ + N], qkv[NQ + N:]

    def temporal_tables(self, p):
        """(rte_k, rte_v): K / V images of the 240 temporal rows per source type (conv.py:91-92,298-299 hoisted off the edges)."""
        T, dp, din, L = self.T, self.dp, self.din, _lib.HGT_RTE_LEN
        rr, ro = _rte_row_lists(T, self.dev)
        rte_lin = self.new(L, din)
        _typed_linear(self.split, p.rte_emb, din, rr.data_ptr(), ro.data_ptr(), 1, L, din, din, p.rte_w, 0, 0, p.rte_b, 0, 0, [rte_lin], din,
                      by_pos=1)
        rte_kv = self.new(2, T * L, dp)
        _typed_linear(self.split, rte_lin, din, rr.data_ptr(), ro.data_ptr(), T, T * L, din, 2 * dp, p.w_qkv, dp * din, 3 * dp * din, None, 0, 0,
                      [rte_kv[0], rte_kv[1]], dp, by_pos=1)
        return rte_kv[0], rte_kv[1]

    def attention(self, Q, K, rte_k, att_t):
        """(att in plan order, self.att of conv.py:108 in the caller's edge order or None): logits (conv.py:98-99), softmax in place."""
        att = self.logits(self.plan, Q, K, rte_k, att_t)
        check(self.lib.hgt_edge_softmax(*self.graph(self.plan), _ptr(att), _stream()), "hgt_edge_softmax")
        keep = self.layer.keep_att and self.E > 0
        return att, (self.to_edge_ids(self.plan, att, out_heads=self.layer.n_heads) if keep else None)

    def aggregate(self, att, V, rte_v, msg_p, msg_f):
        """agg = sum_r (sum_e att_e v_e) M_r (conv.py:104,109-111 + scatter-add)."""
        agg = self.new(self.NQ, self.dp)
        self.spmm(self.plan, att, V.data_ptr(), rte_v, msg_p, msg_f, agg, 0, self.dp, self.NQ)
        return agg

    def a_linear(self, agg, p, mask, gelu):
        """drop(a_linear(gelu(agg))) (HGTConv, conv.py:119-125) or drop(a_linear(agg)) (DenseHGTConv, conv.py:259-261)."""
        trans = self.new(self.NQ, self.dout)
        self.node_linear(agg, self.dp, self.dout, p.w_a, self.dout * self.dp, p.b_a, self.dout, trans, prologue=int(gelu))
        self.drop_(trans, mask)
        return trans

    def update_hgt(self, p, x, agg, m1, m2):
        """HGTConv (conv.py:119-133): a_linear(gelu(agg)) -> dropout -> gated skip -> LayerNorm.  Returns (out, what the backward keeps)."""
        trans = self.a_linear(agg, p, m1, gelu=True)
        out = self.new(self.NQ, self.dout)
        check(self.lib.hgt_node_update(_ptr(trans), _ptr(x), self.din, _ptr(self.plan.node_type), _ptr(p.skip), _ptr(p.ln_w), _ptr(p.ln_b),
                                       int(self.use_norm), self.NQ, self.dout, self.T, _ptr(out), _stream()), "hgt_node_update")
        return out, dict(trans=trans)

    def update_dense(self, p, x, agg, m1, m2):
        """DenseHGTConv (conv.py:250-274): y1 = LN_t(drop(a_linear(agg)) + x); out = out_norm(drop(out_linear(gelu(mid_linear(y1)))) + y1)."""
        lib, N, T, dout, nt = self.lib, self.NQ, self.T, self.dout, _ptr(self.plan.node_type)      # N: the targets
        trans = self.a_linear(agg, p, m1, gelu=False)
        y1 = self.new(N, dout)
        check(lib.hgt_node_update_ex(_ptr(trans), _ptr(x), self.din, nt, None, _ptr(p.ln_w), _ptr(p.ln_b), int(self.use_norm), 0, N, dout, T,
                                     _ptr(y1), _stream()), "hgt_node_update_ex")
        off2 = self.new(2, dtype=torch.int32)                # the target rows of every known type as ONE group (the shared dense layer)
        check(lib.hgt_single_group_offsets(self.rows.off_q, T, _ptr(off2), _stream()), "hgt_single_group_offsets")
        mid = self.new(N, 2 * dout, zero=True)
        _typed_linear(self.split, y1, dout, self.rows.rows_q, off2.data_ptr(), 1, N, dout, 2 * dout, p.mid_w, 0, 0, p.mid_b, 0, 0, [mid], 2 * dout)
        trans2 = self.new(N, dout, zero=True)
        _typed_linear(self.split, mid, 2 * dout, self.rows.rows_q, off2.data_ptr(), 1, N, 2 * dout, dout, p.out_w, 0, 0, p.out_b, 0, 0, [trans2],
                      dout, prologue=1)
        self.drop_(trans2, m2)
        out = self.new(N, dout)
        check(lib.hgt_node_update_ex(_ptr(trans2), _ptr(y1), dout, nt, None, _ptr(p.out_ln_w), _ptr(p.out_ln_b), 1, 1, N, dout, T, _ptr(out),
                                     _stream()), "hgt_node_update_ex")
        return out, dict(trans=trans, y1=y1, mid=mid, trans2=trans2, off2=off2)

    # == backward steps ======================================================================================================
    def a_linear_bwd(self, s, d_trans, gelu):
        """trans = a_linear(f(agg)), f = gelu or identity: (d agg, d w_a, d b_a)."""
        N, dp, dout = self.NQ, self.dp, self.dout      # N: the targets
        a_in = torch.nn.functional.gelu(s.agg) if gelu else s.agg                  # exact erf form, conv.py:119
        d_w_a, d_b_a = _wgrad(self.split, d_trans, dout, a_in, dp, self.rows.rows_q, self.rows.off_q, self.T, N, dout, dp, det=self.det)
        del a_in
        dagg = self.new(N, dp)
        self.node_linear(d_trans, dout, dp, s.w_a.transpose(1, 2).contiguous(), dp * dout, None, 0, dagg)      # [T][dp][dout]
        if gelu:
            dg, dagg = dagg, self.new(N, dp)
            check(self.lib.hgt_gelu_bwd(_ptr(dg), _ptr(s.agg), _ptr(dagg), dagg.numel(), _stream()), "hgt_gelu_bwd")
        # rows of an unknown type get no a_linear (their agg gradient is zero): typed_linear leaves them unwritten
        check(self.lib.hgt_zero_rows(self.rows.rows_q, self.rows.off_q + 4 * self.T, dp, _ptr(dagg), _stream()), "hgt_zero_rows")
        return dagg, d_w_a, d_b_a

    def _ln_grads(self):
        return [self.new(self.T, self.dout, zero=True) if self.use_norm else None for _ in range(2)]

    def update_hgt_bwd(self, s, gout):
        """update_hgt in reverse (conv.py:125-133): (d agg, the skip branch of dx, gradients by slot name)."""
        N, T, din, dout = self.NQ, self.T, self.din, self.dout      # N: the targets
        d_lnw, d_lnb = self._ln_grads()
        d_trans, dx_skip = self.new(N, dout), self.new(N, din)
        d_alpha = self.new(T, zero=True)
        self.node_update_bwd(_ptr(gout), _ptr(s.trans), _ptr(s.x), din, _ptr(self.plan.node_type), _ptr(s.skip), _ptr(s.ln_w),
                             int(self.use_norm), 0, _ptr(s.m1), N, dout, T, _ptr(d_trans), _ptr(dx_skip), din, _ptr(d_alpha), _ptr(d_lnw),
                             _ptr(d_lnb))
        alpha = torch.sigmoid(s.skip)
        d_skip = d_alpha * alpha * (1.0 - alpha)
        dagg, d_w_a, d_b_a = self.a_linear_bwd(s, d_trans, gelu=True)
        return dagg, dx_skip, dict(w_a=d_w_a, b_a=d_b_a, skip=d_skip, ln_w=d_lnw, ln_b=d_lnb)

    def update_dense_bwd(self, s, gout):
        """update_dense in reverse (conv.py:250-274): (d agg, the residual branch of dx, gradients by slot name)."""
        lib, N, T, din, dout, nt = self.lib, self.NQ, self.T, self.din, self.dout, _ptr(self.plan.node_type)      # N: the targets
        rows_q, off2 = self.rows.rows_q, s.off2.data_ptr()
        d_lnw, d_lnb = self._ln_grads()
        d_trans, dx_skip = self.new(N, dout), self.new(N, din)
        d_oln_w, d_oln_b = self.new(1, dout, zero=True), self.new(1, dout, zero=True)
        d_t2 = self.new(N, dout)                                                      # gradient of out_linear's (dropped) output
        d_y1 = self.new(N, dout)                                                      # residual branch of y1
        self.node_update_bwd(_ptr(gout), _ptr(s.trans2), _ptr(s.y1), dout, nt, None, _ptr(s.out_ln_w), 1, 1, _ptr(s.m2), N, dout, T,
                             _ptr(d_t2), _ptr(d_y1), dout, None, _ptr(d_oln_w), _ptr(d_oln_b))
        g2 = torch.nn.functional.gelu(s.mid)
        d_out_w, d_out_b = _wgrad(self.split, d_t2, dout, g2, 2 * dout, rows_q, off2, 1, N, dout, 2 * dout, det=self.det)
        del g2
        out_w_t = s.out_w.t().contiguous()                                            # [2 dout][dout]
        d_g2 = self.new(N, 2 * dout, zero=True)
        _typed_linear(self.split, d_t2, dout, rows_q, off2, 1, N, dout, 2 * dout, out_w_t, 0, 0, None, 0, 0, [d_g2], 2 * dout)
        d_mid = torch.empty_like(d_g2)
        check(lib.hgt_gelu_bwd(_ptr(d_g2), _ptr(s.mid), _ptr(d_mid), d_mid.numel(), _stream()), "hgt_gelu_bwd")
        del d_g2
        d_mid_w, d_mid_b = _wgrad(self.split, d_mid, 2 * dout, s.y1, dout, rows_q, off2, 1, N, 2 * dout, dout, det=self.det)
        mid_w_t = s.mid_w.t().contiguous()                                            # [dout][2 dout]
        d_y1b = self.new(N, dout, zero=True)
        _typed_linear(self.split, d_mid, 2 * dout, rows_q, off2, 1, N, 2 * dout, dout, mid_w_t, 0, 0, None, 0, 0, [d_y1b], dout)
        d_y1 += d_y1b
        del d_mid, d_y1b
        self.node_update_bwd(_ptr(d_y1), _ptr(s.trans), _ptr(s.x), din, nt, None, _ptr(s.ln_w), int(self.use_norm), 0, _ptr(s.m1), N, dout, T,
                             _ptr(d_trans), _ptr(dx_skip), din, None, _ptr(d_lnw), _ptr(d_lnb))
        dagg, d_w_a, d_b_a = self.a_linear_bwd(s, d_trans, gelu=False)
        return dagg, dx_skip, dict(w_a=d_w_a, b_a=d_b_a, ln_w=d_lnw, ln_b=d_lnb, mid_w=d_mid_w[0], mid_b=d_mid_b[0], out_w=d_out_w[0],
                                   out_b=d_out_b[0], out_ln_w=d_oln_w[0], out_ln_b=d_oln_b[0])

    def attention_bwd(self, s, dagg):
        """d s, the gradient of the logits in plan order (conv.py:98-111): d att = <dagg_i M^T, v_e>, rho = <dagg, agg> per head, then the
        softmax backward."""
        plan, N, E, H = self.plan, self.NQ, self.E, self.H      # N: the targets
        ones_pri = torch.full((self.R, self.Hreal), math.sqrt(self.dk), dtype=torch.float32, device=self.dev)      # pri / sqrt(dk) == 1
        m_t, _ = self.pack(s.rmsg, s.rmsg, ones_pri)                                  # m_t[r,h,c,k] = M[r,h,k,c]
        d_att = self.logits(plan, dagg, self.qkv_views(s.qkv)[2], s.rte_v, m_t)
        rho = self.new(N, H)
        check(self.lib.hgt_head_dot(_ptr(dagg), _ptr(s.agg), N, H, self.dkp, _ptr(rho), _stream()), "hgt_head_dot")
        ds = self.new(E, H)
        check(self.lib.hgt_edge_softmax_bwd(*self.graph(plan), _ptr(s.att), _ptr(d_att), _ptr(rho), H, _ptr(ds), _stream()),
              "hgt_edge_softmax_bwd")
        return ds

    def qkv_bwd(self, s, dagg, ds, scale):
        """dqkv [N, 3 dp] by three gather passes: dQ over the plan, dK and dV over the transposed plan.  Also returns the
        (matrices, fragments) of the dK and of the dV pass, which temporal_bwd runs again grouped by table row."""
        plan, dp, N = self.plan, self.dp, self.N
        Q, K, _ = self.qkv_views(s.qkv)
        a_s = s.ratt * scale                                                         # A[k][c] * pri / sqrt(dk)
        dqkv = self.new(N, 3 * dp, zero=True)
        # dQ_i = sum_r (sum_e ds_e k_e) . (A s)           [out = in . F, F[k][c] = A[k][c] s]
        _, f_q = self.pack(s.ratt, a_s, s.rpri)
        self.spmm(plan, ds, K.data_ptr(), s.rte_k, f_q, self.frags(f_q), dqkv, 0, 3 * dp, self.NQ)
        # transposed graph (every node a target, the sources are the original targets: Q and dagg have NQ rows): dK_j = sum_r (sum_e ds_e q_i) . (A s)^T,  dV_j = sum_r (sum_e att_e dagg_i) . M^T
        plan_t = plan.transposed()
        ds_t = self.to_sorted(plan_t, self.to_edge_ids(plan, ds))
        att_tr = self.to_sorted(plan_t, self.to_edge_ids(plan, s.att))
        _, f_k = self.pack(s.ratt, a_s.transpose(2, 3), s.rpri)
        f_k = (f_k, self.frags(f_k))
        self.spmm(plan_t, ds_t, Q.data_ptr(), None, *f_k, dqkv, dp, 3 * dp, N)
        _, f_v = self.pack(s.ratt, s.rmsg.transpose(2, 3), s.rpri)
        f_v = (f_v, self.frags(f_v))
        self.spmm(plan_t, att_tr, dagg.data_ptr(), None, *f_v, dqkv, 2 * dp, 3 * dp, N)
        return dqkv, f_k, f_v

    def relation_bwd(self, s, dagg, ds, scale):
        """Gradients of relation_msg / relation_att / relation_pri: two outer products over the edges + the pri / att chain rule."""
        plan, Hr, dk = self.plan, self.Hreal, self.dk
        Q, K, V = self.qkv_views(s.qkv)
        d_msg = self.outer(plan, s.att, V, s.rte_v, dagg)[:, :Hr, :dk, :dk]      # d relation_msg[r,h,k,c]
        o_att = self.outer(plan, ds, K, s.rte_k, Q)[:, :Hr, :dk, :dk]     # sum ds_e k_e[k] q_i[c]
        return dict(rmsg=d_msg.contiguous(), ratt=o_att * scale, rpri=(o_att * s.ratt).sum(dim=(2, 3)) / math.sqrt(dk))

    def temporal_bwd(self, s, dagg, ds, f_k, f_v):
        """use_RTE: the gradient of the temporal tables is the dK / dV gather passes grouped by (source type, dt) instead of by source.
        Returns (gradients by slot name, the tables' share of d w_qkv[:, dp:3dp])."""
        plan, T, dp = self.plan, self.T, self.dp
        plan_r, tab = plan.rte_plan(T, self.R)
        # (ds and att go to edge order a second time: the two [E, H] copies of qkv_bwd are not kept alive across relation_bwd)
        ds_r = self.to_sorted(plan_r, self.to_edge_ids(plan, ds))
        att_r = self.to_sorted(plan_r, self.to_edge_ids(plan, s.att))
        d_tab = self.new(tab, 2 * dp, zero=True)
        # sources of plan_r are the original TARGETS, shifted by `tab` ids: the row pointer is shifted back
        self.spmm(plan_r, ds_r, self.qkv_views(s.qkv)[0].data_ptr() - 4 * tab * dp, None, *f_k, d_tab, 0, 2 * dp, tab)
        self.spmm(plan_r, att_r, dagg.data_ptr() - 4 * tab * dp, None, *f_v, d_tab, dp, 2 * dp, tab)
        if self.det:
            return self.temporal_chain_det(s, d_tab)
        # tables = (emb W_rte^T + b_rte) W_{k|v}[t]^T: chain rule on [T*240, d] arrays with torch ops (tiny)
        with torch.enable_grad():
            e_, w_, b_ = (t.detach().requires_grad_(True) for t in (s.rte_emb, s.rte_w, s.rte_b))
            wkv = s.w_qkv.detach()[:, dp:3 * dp, :].requires_grad_(True)             # [T][2dp][din]
            lin = e_ @ w_.t() + b_                                                   # [240, din]
            tabs = torch.einsum("pd,tod->tpo", lin, wkv).reshape(T * _lib.HGT_RTE_LEN, 2 * dp)
            ge, gw, gb, gkv = torch.autograd.grad(tabs, [e_, w_, b_, wkv], d_tab)
        return dict(rte_emb=ge, rte_w=gw, rte_b=gb), gkv

    def temporal_chain_det(self, s, d_tab):
        """The chain rule of temporal_bwd on this library's own GEMMs instead of torch's (whose BLAS back end may split the reduction
        dimension across workgroups and add with atomics): tables[t] = lin W_kv[t]^T, lin = emb W_rte^T + b_rte.
        Exact fp32 kernels, like the torch ops they stand in for."""
        T, dp, din, L = self.T, self.dp, self.din, _lib.HGT_RTE_LEN
        rr, ro = _rte_row_lists(T, self.dev)                      # rows 0..239 per type, by position
        rows_tl = torch.arange(T * L, dtype=torch.int32, device=self.dev)
        one = torch.tensor([0, L], dtype=torch.int32, device=self.dev)
        lin = self.new(L, din)
        _typed_linear(False, s.rte_emb, din, rr.data_ptr(), ro.data_ptr(), 1, L, din, din, s.rte_w, 0, 0, s.rte_b, 0, 0, [lin], din, by_pos=1)
        # d W_kv[t] = d_tab[t]^T lin
        gkv, _ = _wgrad(False, d_tab, 2 * dp, lin.repeat(T, 1), din, rows_tl.data_ptr(), ro.data_ptr(), T, T * L, 2 * dp, din,
                        with_colsum=False, det=True)
        # d lin = sum_t d_tab[t] W_kv[t]
        wkv_t = s.w_qkv.detach()[:, dp:3 * dp, :].transpose(1, 2).contiguous()          # [T][din][2dp]
        d_lin_t = self.new(T * L, din)
        _typed_linear(False, d_tab, 2 * dp, rows_tl.data_ptr(), ro.data_ptr(), T, T * L, 2 * dp, din, wkv_t, 0, din * 2 * dp, None, 0, 0,
                      [d_lin_t], din)
        d_lin = d_lin_t.view(T, L, din).sum(dim=0)                                       # (torch's reduce kernels sum in a fixed order)
        gw, gb = _wgrad(False, d_lin, din, s.rte_emb.contiguous(), din, rr.data_ptr(), one.data_ptr(), 1, L, din, din, det=True)
        ge = self.new(L, din)
        _typed_linear(False, d_lin, din, rr.data_ptr(), one.data_ptr(), 1, L, din, din, s.rte_w.t().contiguous(), 0, 0, None, 0, 0, [ge], din)
        return dict(rte_emb=ge, rte_w=gw[0], rte_b=gb[0]), gkv

    def project_bwd(self, s, dqkv, dx_skip, d_w_kv_tables, want_dx):
        """project in reverse (conv.py:96-97,103): d w_qkv, d b_qkv and, if asked for, dx (+ the skip / residual branch)."""
        T, N, NQ, dp, din, rows = self.T, self.N, self.NQ, self.dp, self.din, self.rows
        if NQ < N:
            return self.project_bwd_rect(s, dqkv, dx_skip, d_w_kv_tables, want_dx)
        d_w_qkv, d_b_qkv = _wgrad(self.split, dqkv, 3 * dp, s.x, din, rows.rows_all, rows.off_all, T, N, 3 * dp, din, det=self.det)
        if d_w_kv_tables is not None:
            d_w_qkv[:, dp:3 * dp, :] += d_w_kv_tables
        grads = dict(w_qkv=d_w_qkv, b_qkv=d_b_qkv)
        if want_dx:
            w_qkv_t = s.w_qkv.transpose(1, 2).contiguous()                           # [T][din][3dp]
            dx = self.new(N, din, zero=True)
            _typed_linear(self.split, dqkv, 3 * dp, rows.rows_all, rows.off_all, T, N, 3 * dp, din, w_qkv_t, 0, din * 3 * dp, None, 0, 0, [dx], din)
            dx += dx_skip
            grads["x"] = dx
        return grads

    def project_bwd_rect(self, s, dqkv, dx_skip, d_w_kv_tables, want_dx):
        """project_bwd with source-only rows: the targets' GEMMs read all 3 dp columns of dqkv, those of the rows [NQ, N) its K|V
        block alone (their Q block is zero), and the skip / residual branch exists on the targets only."""
        T, N, NQ, dp, din, rows = self.T, self.N, self.NQ, self.dp, self.din, self.rows
        h_rows, h_off, n_h = self.halo
        d_kv = dqkv[:, dp:]                                                          # [N, 2dp] view, leading dimension 3dp
        d_w_qkv, d_b_qkv = _wgrad(self.split, dqkv, 3 * dp, s.x, din, rows.rows_q, rows.off_q, T, NQ, 3 * dp, din, det=self.det)
        if n_h:
            d_w_h, d_b_h = _wgrad(self.split, d_kv, 3 * dp, s.x, din, h_rows.data_ptr(), h_off.data_ptr(), T, n_h, 2 * dp, din, det=self.det)
            d_w_qkv[:, dp:3 * dp, :] += d_w_h
            d_b_qkv[:, dp:3 * dp] += d_b_h
        if d_w_kv_tables is not None:
            d_w_qkv[:, dp:3 * dp, :] += d_w_kv_tables
        grads = dict(w_qkv=d_w_qkv, b_qkv=d_b_qkv)
        if want_dx:
            dx = self.new(N, din, zero=True)
            w_qkv_t = s.w_qkv.transpose(1, 2).contiguous()                           # [T][din][3dp]
            _typed_linear(self.split, dqkv, 3 * dp, rows.rows_q, rows.off_q, T, NQ, 3 * dp, din, w_qkv_t, 0, din * 3 * dp, None, 0, 0, [dx], din)
            if n_h:
                w_kv_t = s.w_qkv[:, dp:3 * dp, :].transpose(1, 2).contiguous()       # [T][din][2dp]
                _typed_linear(self.split, d_kv, 3 * dp, h_rows.data_ptr(), h_off.data_ptr(), T, n_h, 2 * dp, din, w_kv_t, 0, din * 2 * dp,
                              None, 0, 0, [dx], din)
            dx[:NQ] += dx_skip
            grads["x"] = dx
        return grads


class _HGTConvTrain(torch.autograd.Function):
    """HGTConv / DenseHGTConv forward + backward on the HIP kernels.  The message path (conv.py:60-111) is shared; the update is
    conv.py:114-134 (HGTConv: gelu, a_linear, dropout, gated skip, LayerNorm) or conv.py:250-274 (DenseHGTConv: a_linear, dropout,
    plain residual, LayerNorm, then the shared dense layer with its own dropout and out_norm)."""

    @staticmethod
    def forward(ctx, layer, plan, drop_masks, *tensors):
        p = SimpleNamespace(**dict(zip(TENSOR_SLOTS, tensors)))
        step = _Step(layer, plan, _lib.layout_for(layer.out_dim, layer.n_heads))
        dense = p.mid_w is not None
        x = p.x.contiguous()
        att_t, msg_p, msg_f = step.relation_images(p)
        qkv = step.project(x, p)
        rte_k, rte_v = step.temporal_tables(p) if layer.use_RTE else (None, None)
        Q, K, V = step.qkv_views(qkv)
        att, layer.att = step.attention(Q, K, rte_k, att_t)
        agg = step.aggregate(att, V, rte_v, msg_p, msg_f)
        # drop_masks: None, (m1, m2) float masks, or the _CounterDropout of the recompute mode (sites instead of tensors)
        ctx.drop = drop_masks if isinstance(drop_masks, _CounterDropout) else None
        if ctx.drop is not None:
            m1, m2 = ctx.drop.site(0), ctx.drop.site(1)
        else:
            m1, m2 = drop_masks if drop_masks is not None else (None, None)
        out, kept = (step.update_dense if dense else step.update_hgt)(p, x, agg, m1, m2)
        ctx.layer, ctx.plan, ctx.lay, ctx.dense = layer, plan, step.lay, dense
        ctx.recompute = takes_recompute(layer)
        saved = dict(x=x, w_qkv=p.w_qkv, w_a=p.w_a, ratt=p.ratt, rmsg=p.rmsg, rpri=p.rpri, skip=p.skip, ln_w=p.ln_w,
                     rte_emb=p.rte_emb, rte_w=p.rte_w, rte_b=p.rte_b, mid_w=p.mid_w, out_w=p.out_w, out_ln_w=p.out_ln_w,
                     qkv=qkv, att=att, agg=agg, rte_k=rte_k, rte_v=rte_v, m1=m1, m2=m2, **kept)
        if ctx.recompute:
            # not kept: Q|K|V, the masks and HGTConv's a_linear output (DenseHGTConv's feeds y1, which stays).  The recomputation reads
            # b_qkv and b_a, which the default mode lets go: instead of the packed arrays (new memory) the bias PARAMETERS they were
            # packed from are saved (they live anyway, and torch checks their version counters like any saved tensor's)
            saved.update(qkv=None, m1=None, m2=None)
            if not dense:
                saved.update(trans=None)
            saved.update({"bias_%s%d" % (k, t): b for k, bs in layer._bias_parameters().items() for t, b in enumerate(bs)})
        _save_named(ctx, saved)
        return out

    @staticmethod
    def backward(ctx, gout):
        s = _load_named(ctx)
        step = _Step(ctx.layer, ctx.plan, ctx.lay)
        if ctx.recompute:
            # what the forward did not keep, by the forward's own steps on the forward's inputs (the same kernels, hence the same bits),
            # each dropped after its last consumer.  `s` is rebuilt per call: a second backward (retain_graph) recomputes again
            drop = ctx.drop
            with torch.no_grad():
                s.b_qkv, s.b_a = ctx.layer._pack_biases({k: [getattr(s, "bias_%s%d" % (k, t)) for t in range(step.T)] for k in "qkva"},
                                                        ctx.lay)
            if not ctx.dense:
                s.trans = step.a_linear(s.agg, s, drop and drop.site(0), gelu=True)
            s.m1, s.m2 = (step.drop_mask(drop.site(0)), step.drop_mask(drop.site(1))) if drop else (None, None)
        dagg, dx_skip, grads = (step.update_dense_bwd if ctx.dense else step.update_hgt_bwd)(s, gout.contiguous().float())
        if ctx.recompute:
            s.m1 = s.m2 = None
            if not ctx.dense:
                s.trans = None
            s.qkv = step.project(s.x, s)
        ds = step.attention_bwd(s, dagg)
        scale = (s.rpri / math.sqrt(step.dk)).view(step.R, step.Hreal, 1, 1)
        dqkv, f_k, f_v = step.qkv_bwd(s, dagg, ds, scale)
        grads.update(step.relation_bwd(s, dagg, ds, scale))
        d_w_kv_tables = None
        if ctx.layer.use_RTE:
            rte_grads, d_w_kv_tables = step.temporal_bwd(s, dagg, ds, f_k, f_v)
            grads.update(rte_grads)
        if ctx.recompute:
            s.qkv = None
        grads.update(step.project_bwd(s, dqkv, dx_skip, d_w_kv_tables, ctx.needs_input_grad[len(PLAIN_SLOTS) + TENSOR_SLOTS.index("x")]))
        assert set(grads) <= set(TENSOR_SLOTS), sorted(set(grads) - set(TENSOR_SLOTS))
        return (None,) * len(PLAIN_SLOTS) + tuple(grads.get(k) for k in TENSOR_SLOTS)


def hgt_conv_train(layer, plan, x, packed, drop_p):
    """Training-mode forward of `layer` (HGTConv or DenseHGTConv) through the autograd Function.  `packed` =
    layer._pack_parameters(grad=True); drop_p = dropout probability of conv.py:125 / 261,273 (0 in eval mode).
    plan.NQ < plan.N: nodes [0, NQ) are targets, nodes [NQ, N) source-only rows (a rank of a destination partition): the output is
    [NQ, out_dim], x.grad [N, in_dim] with the K / V paths alone on the rows [NQ, N)."""
    if not 0 <= plan.NQ <= plan.N:
        raise ValueError("pyhgt_amd: the plan's n_q_rows must lie in [0, n_nodes]")
    ok, reason = training_supported(layer.out_dim, layer.n_heads)
    if not ok:      # said HERE instead of failing inside loss.backward()
        raise NotImplementedError("pyhgt_amd: " + reason)
    if plan.NQ == 0 and plan.N > 0:
        # (the edge kernels read n_q_rows = 0 as "all rows"; a step without targets has no output and no gradient anyway)
        raise ValueError("pyhgt_amd: a training step needs at least one target row (n_q_rows == 0 of %d nodes)" % plan.N)
    dense = "mid_w" in packed
    masks = None
    if drop_p > 0.0 and takes_recompute(layer):
        # one 64-bit seed per layer call from torch's CPU generator (torch.manual_seed governs it; no device synchronisation);
        # DenseHGTConv drops twice (conv.py:261 and conv.py:273).  keep <= 0: hgt_dropout_* write zeros, like the rule below
        seed = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) & (2 ** 64 - 1)
        masks = _CounterDropout(seed, float(1.0 - drop_p), tuple(s << DROP_SITE_SHIFT for s in range(2 if dense else 1)))
    elif drop_p > 0.0:
        keep = 1.0 - drop_p
        if keep <= 0.0:      # nn.Dropout(p=1) yields zeros (not 0/0)
            draw = lambda: torch.zeros((plan.NQ, layer.out_dim), dtype=torch.float32, device=x.device)
        else:
            draw = lambda: torch.bernoulli(torch.full((plan.NQ, layer.out_dim), keep, dtype=torch.float32, device=x.device)) / keep
        masks = (draw(), draw() if dense else None)          # DenseHGTConv drops twice (conv.py:261 and conv.py:273)
    if takes_recompute(layer):      # (seed, keep, offsets) of this call's dropout, for whoever wants its masks again; None: no dropout
        layer.last_dropout_state = tuple(masks) if masks is not None else None
    inputs = dict(packed, x=x)
    assert all(k in TENSOR_SLOTS for k, t in inputs.items() if torch.is_tensor(t)), "a packed parameter without a slot in TENSOR_SLOTS"
    return _HGTConvTrain.apply(layer, plan, masks, *(inputs.get(k) for k in TENSOR_SLOTS))


class TypedLinearFunction(torch.autograd.Function):
    """y[n] = x[n] W[type(n)]^T + b[type(n)] on the typed-linear kernels with its backward (typed weight gradient, column
    sums, optional input gradient): the input adapter of model.GNN (model.py:70-76) and the Linear layers of the heads."""

    @staticmethod
    def forward(ctx, plan_rows, n_groups, precision, x, w, b, deterministic=False):
        # plan_rows = (rows ptr, off ptr, keep-alive object); w [G][n_out][k], b [G][n_out]
        rows, off, _keep = plan_rows
        x = x.contiguous()
        n, k = x.shape
        n_out = w.shape[1]
        y = torch.zeros(n, n_out, dtype=torch.float32, device=x.device)
        wc, bc = w.contiguous(), (b.contiguous() if b is not None else None)
        _typed_linear(precision in _SPLIT, x, k, rows, off, n_groups, n, k, n_out, wc, 0, n_out * k, bc, 0, n_out, [y], n_out)
        ctx.plan_rows, ctx.n_groups, ctx.has_bias, ctx.split = plan_rows, n_groups, b is not None, precision in _SPLIT
        ctx.det = bool(deterministic)
        ctx.save_for_backward(x, wc)
        return y

    @staticmethod
    def backward(ctx, gy):
        rows, off, _keep = ctx.plan_rows
        x, w = ctx.saved_tensors
        G = ctx.n_groups
        gy = gy.contiguous().float()
        n, k = x.shape
        n_out = w.shape[1]
        dw, db = _wgrad(ctx.split, gy, n_out, x, k, rows, off, G, n, n_out, k, with_colsum=ctx.has_bias, det=ctx.det)
        dx = None
        if ctx.needs_input_grad[3]:
            wt = w.transpose(1, 2).contiguous()
            dx = torch.zeros(n, k, dtype=torch.float32, device=x.device)
            # split=False for every precision, unlike the layer's own data gradients: this input gradient has always run on the exact
            # fp32 kernel (the heads are 'fp32' anyway; the adapter's is asked for only when the features themselves require grad),
            # and moving it to the split kernel would change results
            _typed_linear(False, gy, n_out, rows, off, G, n, n_out, k, wt, 0, k * n_out, None, 0, 0, [dx], k)
        return None, None, None, dx, dw, db, None
