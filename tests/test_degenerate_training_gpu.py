"""GPU tests of the training step (pyhgt_amd/autograd.py) on edgeless, single-edge and sub-wavefront graphs: HGTConv / DenseHGTConv
forward + backward under grad, and a two-layer GNN + Classifier step, against the fp64 oracle (oracle.hgt_oracle).  The graphs are
written out by hand below (GRAPHS) so that each degenerate property is visible; tests/test_degenerate_training.py runs the oracle
side and the classification rule on the CPU.

What is asserted, and against what:

(a) forward: max |out - forward_closed_form| < FWD_TOL = 1e-4 (the project's bound); rows of an unknown node type are bit-zero.
(b) gradients of x and of every parameter: test_backward_gpu._grads_close (2e-4 of the tensor's largest oracle entry + the per-entry
    bound; imported, not copied).  Those bounds are relative to the tensor's own scale and say nothing where the oracle gradient is
    zero, which on these graphs is most tensors.  Every entry of every gradient is therefore classified FROM THE GRAPH (entry_kinds;
    never from the kernels' result) as
      STRUCTURAL -- nothing feeds it: a type without a target row (a_linears, norms, skip), a type whose target rows have no claimed
          in-edge (q_linears; a_linears.weight, whose input gelu(agg) / agg is then zero), a type without a row that is the source
          of a claimed edge (k_linears, v_linears), a relation without a claimed edge (its slices of relation_att / _msg / _pri),
          emb.* without any claimed edge, rows of x of an unknown type or source-only without a claimed out-edge.  (An edge is
          claimed when both end types lie in [0, T) and its relation in [0, R): the others keep logit 0 and carry no message,
          conv.py:68-69.)  These entries must be finite and BIT-ZERO.
      CANCELLING -- every claimed edge that feeds the entry is the only in-edge of its target: the softmax over one entry is the
          constant 1, so d logit = att (d att - rho) vanishes in exact arithmetic (|oracle| <= 1e-12 of the sibling scale below is
          asserted) but not in fp32, where d att comes from the logits kernel and rho = <d agg, agg> from an aggregate computed
          with split-bf16 relation transforms (~1e-5 of d att).  Touches q_linears, k_linears, relation_att, relation_pri.
          Bounded by RTOL = 2e-4 (test_backward_gpu.RTOL) of the scale of the sibling that does not cancel:
            q / k_linears.*.weight (.bias): the largest oracle entry over v_linears.*.weight (.bias);
            relation_att: B_att = RTOL * the largest oracle entry of relation_msg;
            relation_pri: d pri[r,h] = sum_kc d att[r,h,k,c] att[r,h,k,c] / pri[r,h] (the chain rule of _Step.relation_bwd:
                d att = o_att * pri / sqrt(dk), d pri = sum(o_att * att) / sqrt(dk)), hence
                |d pri[r,h]| <= B_att * sum_kc |att[r,h,k,c]| / |pri[r,h]|, maximised over the cancelling (r, h).
          The measured ratio (largest |entry| / bound) is printed per case.
      REGULAR -- everything else; the oracle gradient of every regular slice must be non-zero (asserted: a wrong rule fails here,
          on the oracle's numbers), and the tensor goes through _grads_close.
(c) unwritten outputs: before every step the caching allocator is poisoned (_poison: 60 MB of blocks of the sizes a step asks for,
    filled with NaN and dropped without empty_cache), so that the step's torch.empty outputs -- all reduction outputs of the
    deterministic route, agg / d agg / d s on both -- come back full of NaN and a slot no kernel writes fails (a) or (b).
(d) the deterministic route run twice gives equal bits for the output and every gradient.
(e) the recompute mode (set_recompute) gives the bits of the default mode (drop probability 0).

The bounds are also recorded in DESIGN.md section 7 (backward parity).
"""
import math

import pytest
import torch

import test_backward_gpu as BG
from oracle import hgt_oracle as O
from pyhgt_amd import Classifier, DenseHGTConv, GNN, GraphPlan, HGTConv, set_deterministic, set_recompute

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 1e-4
T, R = 3, 4
REGULAR, STRUCTURAL, CANCELLING = 0, 1, 2


# == the graphs ====================================================================================================================
def _i64(v):
    return torch.tensor(v, dtype=torch.int64)


def _edges(pairs):
    """[2, E] int64 from (source, target) pairs; E = 0 gives the empty [2, 0] tensor a sampler hands over."""
    return _i64(pairs).t().contiguous() if pairs else torch.zeros(2, 0, dtype=torch.int64)


def _random_edges(n_edges, n_src, n_dst, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack([torch.randint(0, n_src, (n_edges,), generator=g), torch.randint(0, n_dst, (n_edges,), generator=g)])
    return ei, torch.randint(0, R, (n_edges,), generator=g), torch.randint(0, 240, (n_edges,), generator=g)


def _graphs():
    """name -> dict(nt, ei, et, tm, NQ, use_norm, use_RTE).  T = 3 types and R = 4 relations throughout."""
    G = {}

    def add(name, nt, ei, et, tm, NQ=None, use_norm=True, use_RTE=True):
        nt = _i64(nt)
        G[name] = dict(name=name, nt=nt, ei=ei, et=_i64(et) if not torch.is_tensor(et) else et,
                       tm=_i64(tm) if not torch.is_tensor(tm) else tm, NQ=nt.numel() if NQ is None else NQ, use_norm=use_norm,
                       use_RTE=use_RTE)

    # every per-edge array empty; transposed() and rte_plan() of an empty edge list
    add("no_edges", [0, 0, 1, 2, 2], _edges([]), [], [])
    # one row: fewer rows than the 4-row workgroups of the row kernels and than a 64-row GEMM tile
    add("one_node_no_edge", [0], _edges([]), [], [])
    # one work item of one edge; a softmax over one entry
    add("one_node_self_loop", [1], _edges([(0, 0)]), [2], [7])
    # the last relation, the last temporal row, source type != target type; type 2 has no node
    add("single_edge", [0, 1], _edges([(0, 1)]), [R - 1], [239])
    # type 1 has no node (an empty row list between two non-empty ones); 200 edges into the targets 0..19: 43 targets without
    # in-edges; N one short of a wavefront
    ei, et, tm = _random_edges(200, 63, 20, seed=101)
    nt63 = [0] * 30 + [2] * 33
    add("empty_type_isolated", nt63, ei, et, tm)
    # the unclaimed bucket alone: logit 0, no message, still in the softmax
    add("all_unclaimed", nt63, ei, torch.full_like(et, R), tm)
    # R - 1 relations without an edge (their relation_* gradient slots); no temporal tables, no LayerNorm
    add("one_relation", nt63, ei, torch.full_like(et, 2), tm, use_norm=False, use_RTE=False)
    # equal keys in the plan's sort and in the transposed plan: five edges into node 1, four of them identical
    add("duplicates", [0, 1, 2], _edges([(0, 1)] * 4 + [(2, 1)]), [1, 1, 1, 1, 0], [5, 5, 5, 5, 9])
    # one row past a 64-row tile, and that row is of an unknown type (T + 1); edges from and into it are unclaimed
    ei, et, tm = _random_edges(300, 65, 65, seed=102)
    g = torch.Generator().manual_seed(103)
    add("ragged_65", torch.randint(0, T, (64,), generator=g).sort().values.tolist() + [T + 1], ei, et, tm)
    # rectangular steps (a rank of a destination partition): targets 0, 1; source-only rows [known, known, unknown type, referenced
    # by no edge]
    rect_edges = _edges([(2, 0), (3, 0), (3, 1), (4, 1), (0, 1), (1, 0), (2, 1), (2, 0)])
    rect_et, rect_tm = [0, 1, 2, 3, 1, 0, 3, 0], [0, 17, 239, 5, 100, 3, 64, 1]
    add("rect_halo_mixed", [0, 1, 0, 2, T + 1, 1], rect_edges, rect_et, rect_tm, NQ=2)
    # ... and with all four source-only rows of an unknown type: halo_row_lists() returns no row
    add("rect_halo_unknown", [0, 1, T + 1, T + 1, T + 1, T + 1], rect_edges, rect_et, rect_tm, NQ=2)
    return G


GRAPHS = _graphs()
SQUARE = ["no_edges", "one_node_no_edge", "one_node_self_loop", "single_edge", "empty_type_isolated", "all_unclaimed", "one_relation",
          "duplicates", "ragged_65"]
RECT = ["rect_halo_mixed", "rect_halo_unknown"]


# == the classification rule (computed from the graph alone) =========================================================================
def graph_facts(g):
    """What the rule needs: per type / relation, the claimed edges that feed it and whether each of them is the only in-edge of its
    target (`lonely`)."""
    nt, ei, et, NQ = g["nt"], g["ei"], g["et"], g["NQ"]
    N = nt.numel()
    src, dst = ei[0], ei[1]
    known = (nt >= 0) & (nt < T)
    claimed = known[src] & known[dst] & (et >= 0) & (et < R)
    indeg = torch.bincount(dst, minlength=N)
    lonely = indeg[dst] == 1                                   # unclaimed in-edges sit in the softmax too
    return dict(N=N, NQ=NQ, known=known, claimed=claimed, lonely=lonely, src=src, dst=dst, et=et, nt=nt,
                target_types={int(t) for t in nt[:NQ][known[:NQ]]})


def _kind_of(edge_sel, f):
    """Kind of an entry fed through the logits of the claimed edges `edge_sel` alone."""
    sel = edge_sel & f["claimed"]
    if not bool(sel.any()):
        return STRUCTURAL
    return CANCELLING if bool(f["lonely"][sel].all()) else REGULAR


def entry_kinds(g, key, shape):
    """int tensor broadcastable to `shape`: the kind of every entry of the gradient named `key` ("x" or a state_dict name)."""
    f = graph_facts(g)
    nt, src, dst, et, claimed = f["nt"], f["src"], f["dst"], f["et"], f["claimed"]
    scalar = lambda k: torch.tensor(k)
    parts = key.split(".")
    if key == "x":
        kinds = torch.full((f["N"], 1), STRUCTURAL)
        kinds[:f["NQ"]][f["known"][:f["NQ"]]] = REGULAR          # a known target row: skip / residual branch
        kinds[src[claimed]] = REGULAR                           # K and V of a claimed edge's source
        return kinds
    if parts[0] in ("a_linears", "norms"):
        t = int(parts[1])
        if t not in f["target_types"]:
            return scalar(STRUCTURAL)
        if parts[0] == "a_linears" and parts[2] == "weight":    # its input is gelu(agg) (HGTConv) or agg (DenseHGTConv): zero rows
            return scalar(REGULAR if bool((claimed & (nt[dst] == t)).any()) else STRUCTURAL)
        return scalar(REGULAR)
    if key == "skip":
        return torch.tensor([REGULAR if t in f["target_types"] else STRUCTURAL for t in range(T)])
    if parts[0] == "q_linears":
        return scalar(_kind_of(nt[dst] == int(parts[1]), f))
    if parts[0] == "k_linears":
        return scalar(_kind_of(nt[src] == int(parts[1]), f))
    if parts[0] == "v_linears":                                 # the message path does not cancel
        return scalar(REGULAR if bool((claimed & (nt[src] == int(parts[1]))).any()) else STRUCTURAL)
    if key in ("relation_att", "relation_pri"):
        return torch.tensor([_kind_of(et == r, f) for r in range(R)]).view(R, *([1] * (len(shape) - 1)))
    if key == "relation_msg":
        return torch.tensor([REGULAR if bool((claimed & (et == r)).any()) else STRUCTURAL for r in range(R)]).view(R, 1, 1, 1)
    if parts[0] == "emb":                                       # through K (may cancel) AND through V (does not)
        return scalar(REGULAR if bool(claimed.any()) else STRUCTURAL)
    if parts[0] in ("mid_linear", "out_linear", "out_norm"):    # the shared dense layer: every known target row
        return scalar(REGULAR if f["target_types"] else STRUCTURAL)
    raise KeyError(key)


def cancel_bound(key, sd, ref, kinds):
    """Bound of the CANCELLING entries of `key`: RTOL of the scale of the sibling that does not cancel (module docstring)."""
    parts = key.split(".")
    if parts[0] in ("q_linears", "k_linears"):
        return BG.RTOL * max(ref["v_linears.%d.%s" % (t, parts[2])].abs().max().item() for t in range(T))
    b_att = BG.RTOL * ref["relation_msg"].abs().max().item()
    if key == "relation_att":
        return b_att
    if key == "relation_pri":
        # |d pri[r,h]| <= B_att * sum_kc |att[r,h,k,c]| / |pri[r,h]| over the cancelling relations
        w = sd["relation_att"].double().abs().sum(dim=(2, 3)) / sd["relation_pri"].double().abs()
        return b_att * w[(kinds == CANCELLING).view(R)].max().item()
    raise KeyError("no cancelling rule for " + key)


def check_rule_against_oracle(g, sd, ref):
    """The rule's statements about the ORACLE gradients (CPU only): finite; structural entries exactly zero; cancelling entries below
    1e-12 of their bound's scale; every regular slice non-zero."""
    for key, r in ref.items():
        assert bool(torch.isfinite(r).all()), key
        kinds = entry_kinds(g, key, r.shape).expand(r.shape)
        assert bool((r[kinds == STRUCTURAL] == 0).all()), "%s / %s: the oracle is non-zero on an entry the rule calls structural" % (
            g["name"], key)
        if bool((kinds == CANCELLING).any()):
            bound = cancel_bound(key, sd, ref, entry_kinds(g, key, r.shape))
            assert bound > 0, (g["name"], key)
            assert r[kinds == CANCELLING].abs().max().item() <= 1e-12 * bound / BG.RTOL, (g["name"], key)
        k0 = entry_kinds(g, key, r.shape)
        if k0.dim() == 0:
            slices = [r] if int(k0) == REGULAR else []
        else:
            lead = k0.reshape(k0.shape[0], -1)[:, 0]
            slices = [r[i] for i in range(r.shape[0]) if int(lead[i]) == REGULAR]
        for s in slices:
            assert s.abs().max().item() > 0, "%s / %s: the oracle is zero on a slice the rule calls regular" % (g["name"], key)


# == the oracle side: computed once per (graph, layout, layer kind), shared, never modified ======================================
_REF = {}


def reference(name, d, H, dense=False):
    key = (name, d, H, dense)
    if key not in _REF:
        g = GRAPHS[name]
        N = g["nt"].numel()
        sd = O.make_state_dict(d, d, T, R, H, g["use_norm"], g["use_RTE"], seed=301, dense=dense)
        gen = torch.Generator().manual_seed(302 + N)
        x = torch.randn(N, d, generator=gen)
        gout = torch.zeros(N, d)
        gout[:g["NQ"]] = torch.randn(g["NQ"], d, generator=gen)          # zero on the source-only rows
        tm = g["tm"] if g["use_RTE"] else None
        kw = dict(use_norm=g["use_norm"], use_RTE=g["use_RTE"], dense=dense)
        fwd = O.forward_closed_form(sd, T, R, H, x, g["nt"], g["ei"], g["et"], tm, **kw)
        ref = O.backward_reference(sd, T, R, H, x, g["nt"], g["ei"], g["et"], tm, gout, **kw)
        _REF[key] = (sd, x, gout, fwd, ref)
    return _REF[key]


# == (c) the poisoned allocator ====================================================================================================
# bytes x count: the large pool (workspaces, Q|K|V at d = 256, the det partials) and the small pool down to one 512-byte block.  The
# counts fill whole allocator segments (a segment of its own from 10 MB on, 20 MB segments below, 2 MB segments up to 1 MB), so
# that no segment keeps an unpoisoned tail.  60 MB in all
POISON = [(24 << 20, 1), (4 << 20, 4), (2 << 20, 2), (1 << 20, 8), (256 << 10, 16), (32 << 10, 64), (4 << 10, 384), (512, 1024)]


def _poison():
    """Hand every cached block back to the device, then leave 60 MB of NaN-filled blocks in the caching allocator: the torch.empty
    calls of the next step are served from them (no empty_cache after the fill)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    blocks = [torch.empty(nbytes // 4, dtype=torch.float32, device=DEV) for nbytes, count in POISON for _ in range(count)]
    for b in blocks:
        b.fill_(float("nan"))
    torch.cuda.synchronize()
    del blocks


def test_the_poison_reaches_torch_empty():
    """The premise of (c): after _poison, fresh torch.empty blocks of the sizes a tiny step asks for are full of NaN."""
    _poison()
    sizes = (3, 64, 5 * 64, 3 * 64 * 64, 4 * 4 * 16 * 16, 3 * 768 * 256, 63 * 3 * 256)
    fresh = [torch.empty(n, dtype=torch.float32, device=DEV) for n in sizes]      # all of them before the checks' own temporaries
    for n, t in zip(sizes, fresh):
        assert bool(torch.isnan(t).all()), n


# == one step ======================================================================================================================
def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def run_step(name, d, H, conv="hgt", precision="bf16x3", det=False, recompute=False):
    """One eval-mode forward + backward under grad on the device, from a poisoned allocator.  Returns (out, {name: gradient})."""
    g = GRAPHS[name]
    sd, x, gout, _, _ = reference(name, d, H, dense=conv == "dense")
    cls = DenseHGTConv if conv == "dense" else HGTConv
    layer = cls(d, d, T, R, H, 0.2, g["use_norm"], g["use_RTE"], precision=precision).eval()      # eval: no dropout, like the oracle
    layer.load_state_dict(sd)
    layer = layer.to(DEV)
    if det:
        set_deterministic(layer)
    if recompute:
        set_recompute(layer)
    xd = x.to(DEV).requires_grad_(True)
    graph = [g["nt"].to(DEV), g["ei"].to(DEV), g["et"].to(DEV), g["tm"].to(DEV) if g["use_RTE"] else None]
    go = gout[:g["NQ"]].to(DEV)
    GraphPlan.clear_cache()
    _poison()
    out = layer(xd, *graph, n_q_rows=g["NQ"] if g["NQ"] < g["nt"].numel() else None)
    out.backward(go)
    torch.cuda.synchronize()
    grads = {"x": xd.grad}
    for k, p in layer.named_parameters():
        assert p.grad is not None, k
        grads[k] = p.grad
    return out.detach(), grads


def check_step(label, name, d, H, conv, out, grads):
    """(a) and (b) of the module docstring.  Returns the largest (|cancelling entry| / its bound) of the case, or None."""
    g = GRAPHS[name]
    sd, x, gout, fwd, ref = reference(name, d, H, dense=conv == "dense")
    NQ, nt = g["NQ"], g["nt"]
    assert out.shape == (NQ, d)
    o = out.cpu()
    assert bool(torch.isfinite(o).all()), "%s: the output is not finite" % label
    ferr = (o.double() - fwd[:NQ]).abs().max().item()
    print("%s: forward error %.2e" % (label, ferr))
    assert ferr < FWD_TOL, "%s: forward error %.3e" % (label, ferr)
    unknown = ((nt < 0) | (nt >= T))[:NQ]
    assert bool((_bits(o[unknown]) == 0).all()), "%s: a row of an unknown type is not bit-zero" % label
    assert set(grads) == set(ref), (sorted(set(grads) ^ set(ref)))
    worst_cancel = None
    for key in sorted(grads):
        got, r = grads[key].detach().cpu(), ref[key]
        assert got.shape == r.shape, (key, got.shape, r.shape)
        assert bool(torch.isfinite(got).all()), "%s: %s is not finite" % (label, key)
        k0 = entry_kinds(g, key, r.shape)
        kinds = k0.expand(r.shape)
        assert bool((_bits(got)[kinds == STRUCTURAL] == 0).all()), "%s: %s is not bit-zero where nothing feeds it" % (label, key)
        if bool((kinds == CANCELLING).any()):
            bound = cancel_bound(key, sd, ref, k0)
            ratio = got[kinds == CANCELLING].abs().max().item() / bound
            print("%s: cancelling %s: largest entry = %.3f of its bound %.3e" % (label, key, ratio, bound))
            worst_cancel = max(worst_cancel or 0.0, ratio)
            assert ratio <= 1.0, "%s: %s: a cancelling entry is %.3f of its bound %.3e" % (label, key, ratio, bound)
        if bool((kinds == REGULAR).any()):
            BG._grads_close("%s: %s" % (label, key), got, r)
    return worst_cancel


# == 2. the layer matrix ===========================================================================================================
MATRIX = [("hgt", "bf16x3", False), ("hgt", "bf16x3", True), ("dense", "bf16x3", False), ("dense", "bf16x3", True), ("hgt", "fp32", False)]


@pytest.mark.parametrize("conv,precision,det", MATRIX, ids=["%s-%s-%s" % (c, p, "det" if d else "atomic") for c, p, d in MATRIX])
@pytest.mark.parametrize("name", SQUARE)
def test_degenerate_step_matches_the_oracle(name, conv, precision, det):
    label = "%s / %s %s %s" % (name, conv, precision, "det" if det else "atomic")
    out, grads = run_step(name, 64, 4, conv, precision, det)
    check_step(label, name, 64, 4, conv, out, grads)


# d = 200: d_k = 50 pads to 64; d = 16 / one head; d = 256 / two heads: dk_pad 128, hgt_edge_logits_mfma + hgt_relation_outer_wide
LAYOUTS = [(200, 4, "single_edge"), (200, 4, "empty_type_isolated"), (16, 1, "duplicates"), (256, 2, "no_edges"), (256, 2, "single_edge"),
           (256, 2, "empty_type_isolated")]


@pytest.mark.parametrize("d,H,name", LAYOUTS, ids=["d%d_h%d-%s" % c for c in LAYOUTS])
def test_degenerate_step_in_other_layouts(d, H, name):
    from pyhgt_amd import _lib
    from pyhgt_amd.autograd import logits_form, outer_form
    dkp = _lib.layout_for(d, H).dk_pad
    assert dkp == {200: 64, 16: 64, 256: 128}[d]      # (one head takes all 64 lanes: its 16 columns pad to 64 as well)
    assert (logits_form(dkp), outer_form(dkp)) == (("mfma", "hgt_relation_outer_wide") if d == 256 else ("valu", "hgt_relation_outer"))
    out, grads = run_step(name, d, H)
    check_step("%s / d=%d H=%d" % (name, d, H), name, d, H, "hgt", out, grads)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("name", RECT)
def test_rectangular_degenerate_step_matches_the_oracle(name, det):
    """n_q_rows < N (N = 6, NQ = 2): the oracle is the whole graph with a zero grad_out on the source-only rows, as in
    tests/test_partition_training_gpu.py."""
    g = GRAPHS[name]
    if name == "rect_halo_unknown":
        assert not bool(((g["nt"][g["NQ"]:] >= 0) & (g["nt"][g["NQ"]:] < T)).any())      # halo_row_lists: no row
    out, grads = run_step(name, 64, 4, det=det)
    assert grads["x"].shape == (g["nt"].numel(), 64)
    check_step("%s / %s" % (name, "det" if det else "atomic"), name, 64, 4, "hgt", out, grads)


THREE = ["no_edges", "single_edge", "empty_type_isolated"]


@pytest.mark.parametrize("name", THREE)
def test_deterministic_degenerate_step_repeats_bit_for_bit(name):
    o0, g0 = run_step(name, 64, 4, det=True)
    o1, g1 = run_step(name, 64, 4, det=True)
    assert torch.equal(_bits(o0), _bits(o1))
    for k in g0:
        assert torch.equal(_bits(g0[k]), _bits(g1[k])), "%s differs between two runs" % k


@pytest.mark.parametrize("name", THREE)
def test_recompute_gives_the_bits_of_the_default_mode_on_degenerate_graphs(name):
    """Drop probability 0 (eval mode).  On the deterministic route, where the default mode itself repeats."""
    o0, g0 = run_step(name, 64, 4, det=True)
    o1, g1 = run_step(name, 64, 4, det=True, recompute=True)
    check_step("%s / recompute" % name, name, 64, 4, "hgt", o1, g1)
    assert torch.equal(_bits(o0), _bits(o1))
    for k in g0:
        assert torch.equal(_bits(g0[k]), _bits(g1[k])), "%s differs between the modes" % k


# == (e) a whole model =============================================================================================================
def gnn_reference(name, in_dim, d, H, n_cls):
    """(parameters by name, x, labels, fp64 loss, fp64 gradients by name) of a 2-layer GNN + Classifier step whose loss takes every
    node: autograd through the oracle composed like model.py:66-80."""
    g = GRAPHS[name]
    N = g["nt"].numel()
    sd = O.make_gnn_state_dict(in_dim, d, T, R, H, 2, True, True, True, seed=7)
    gen = torch.Generator().manual_seed(401)
    b = 1.0 / math.sqrt(d)
    sd["head.linear.weight"] = (torch.rand((n_cls, d), generator=gen) * 2 - 1) * b
    sd["head.linear.bias"] = (torch.rand((n_cls,), generator=gen) * 2 - 1) * b
    x = torch.randn(N, in_dim, generator=gen)
    y = torch.randint(0, n_cls, (N,), generator=gen)
    P = {k: v.double().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    gnn_sd = {k: v for k, v in P.items() if not k.startswith("head.")}
    h = O.gnn_forward(gnn_sd, in_dim, d, T, R, H, 2, True, True, True, x, g["nt"], g["tm"], g["ei"], g["et"])
    loss = torch.nn.functional.nll_loss(torch.log_softmax(h @ P["head.linear.weight"].T + P["head.linear.bias"], dim=-1), y)
    names = list(P)
    grads = torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)
    return sd, x, y, loss.item(), {k: (gr if gr is not None else torch.zeros_like(P[k])).detach() for k, gr in zip(names, grads)}


def gnn_entry_kinds(g, key, shape):
    """The rule for the model's parameters: an adapter is fed by the rows of its type, the head by every row, a layer's parameters
    as entry_kinds says (every node is a target of both layers and every known row of the first layer's output carries gradient)."""
    if key.startswith("adapt_ws."):
        return torch.tensor(REGULAR if bool((g["nt"] == int(key.split(".")[1])).any()) else STRUCTURAL)
    if key.startswith("head."):
        return torch.tensor(REGULAR)
    return entry_kinds(g, key.split(".", 3)[3], shape)


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("name", ["empty_type_isolated", "no_edges"])
def test_gnn_training_step_on_degenerate_graphs(name, det):
    """Adapter (TypedLinearFunction with an empty group: type 1 has no node) + 2 x HGTConv + Classifier, the loss over every node;
    gradient bound: _grads_close at the 5e-4 of test_gnn_training_step_matches_autograd_through_the_oracle."""
    g = GRAPHS[name]
    in_dim, d, H, n_cls = 37, 64, 4, 5
    sd, x, y, ref_loss, ref = gnn_reference(name, in_dim, d, H, n_cls)
    gnn = GNN(in_dim, d, T, R, H, 2, dropout=0.0, prev_norm=True, last_norm=True, use_RTE=True, deterministic=det)
    head = Classifier(d, n_cls, deterministic=det)
    gnn.load_state_dict({k: v for k, v in sd.items() if not k.startswith("head.")})
    head.load_state_dict({k[len("head."):]: v for k, v in sd.items() if k.startswith("head.")})
    gnn, head = gnn.to(DEV).train(), head.to(DEV).train()
    graph = [t.to(DEV) for t in (g["nt"], g["tm"], g["ei"], g["et"])]
    xd, yd = x.to(DEV), y.to(DEV)
    GraphPlan.clear_cache()
    _poison()
    loss = torch.nn.functional.nll_loss(head(gnn(xd, *graph)), yd)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - ref_loss) < FWD_TOL
    params = dict(list(gnn.named_parameters()) + [("head." + k, v) for k, v in head.named_parameters()])
    assert set(params) == set(ref)
    worst = 0.0
    for key, p in sorted(params.items()):
        assert p.grad is not None, key
        got, r = p.grad.detach().cpu(), ref[key]
        assert bool(torch.isfinite(got).all()), key
        kinds = gnn_entry_kinds(g, key, r.shape).expand(r.shape)
        assert bool((r[kinds == STRUCTURAL] == 0).all()), key
        assert not bool((kinds == CANCELLING).any()), key          # neither graph has a target with exactly one in-edge ... checked here
        assert bool((_bits(got)[kinds == STRUCTURAL] == 0).all()), "%s is not bit-zero where nothing feeds it" % key
        if bool((kinds == REGULAR).any()):
            worst = max(worst, BG._grads_close(key, got, r, rtol=5e-4))
    print("GNN step on %s (%s): worst relative gradient error %.2e" % (name, "det" if det else "atomic", worst))
