"""The one-call forward (hgt_conv_forward, stage 0) on both sides of every size line of its route, against float64.

Conv::route() (pyhgt_amd/csrc/hgt_api.hip) picks the logits kernel, one of the aggregation forms and one of the update forms once per
call, and the kernels it picks make further size decisions of their own (edges per work item, targets per wavefront).  _forward_route
restates all of that in Python; its constants are READ FROM THE SOURCES (and compared with the values restated below), so a retuned
threshold moves the route of the matching case and its `expect` assertion fails loudly instead of silently testing the other side.
The CPU tests (no marker) check _forward_route against hand-derived rows and every case of the GPU list against the side it names;
the GPU tests (marker gpu) run each case with default flags and compare ~2000 rows with the fp64 closed form.

The route cannot be read back from the library.  Where the expected form and its neighbour round differently (merge+update against
two calls, fused against unfused, item-parallel against sub-tile) the case also runs with the flags that force the expected form
and requires the default output to equal it bit for bit.  That proves nothing about lines between forms that are bit-identical or
have no forcing flag (targets per wavefront of the merge+update and sub-tile kernels, edges per work item): there the predicate
comes from the sources alone and the check is the fp64 comparison.

The logits kernel has a line of its own: hgt_edge_logits_kside from 64-edge work items on, where it covers the layer (`logits` is one
of "kside" | "mfma" | "valu").  It rounds differently from the target-side kernels, so the cases that keep the attention weights
run with it forced on and off as well and the default weights must carry the bits of the kernel the route names."""
import os
import re
import time

import pytest
import torch

from oracle import hgt_oracle as O
from pyhgt_amd import GraphPlan, HGTConv, _lib
from pyhgt_amd.synth import induced_in_neighbourhood, pick_check_targets
from test_hgt_gpu import DEV, PREC_TOL, _fp64_rows, _layer_from

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyhgt_amd", "csrc")
ATT_TOL = 1e-5

# constants of the code under test, restated (test_restated_constants_match_the_sources compares them with the sources)
RESTATED = dict(
    FUSED_MIN_NODES=16384,          # hgt_api.hip HGT_FUSED_MIN_NODES: targets from which aggregation + update are one kernel
    ITEM_AGG_MAX_NODES=65536,       # hgt_api.hip: N below this gets the item-parallel scratch, NQ below this may take the form
    ITEM_AGG_DEFAULT_NODES=65536,   # hgt_api.hip: ... and takes it by default
    ITEM_SCRATCH_MAX_LOG2=30,       # hgt_api.hip conv_workspace: zb <= 1 << 30
    ITEM_MAX_RELATIONS=64,          # hgt_api.hip route(): R < 64 (aggregate_items_impl: R >= 64 unsupported)
    FUSED_MAX_DP=256,               # hgt_api.hip route(): fused form for rows of <= 256 padded columns
    MERGE_UPDATE_MAX_DP=512,        # hgt_api.hip route(): merge+update for rows of <= 512 padded columns
    MERGE_UPDATE_MAX_DOUT=512,
    UPDATE_FUSED_DOUT=256,          # hgt_api.hip route(): fuse_update = dout <= 256 || (dout <= 512 && dp <= 512)
    UPDATE_WIDE_DOUT=512,
    UPDATE_WIDE_DP=512,
    MFMA_LOGITS_MIN_DKP=64,         # hgt_api.hip route(): matrix-core logits from d_k (padded) 64 on
    ITEM_MAX_VF=8,                  # hgt_edge_agg_items.hip aggregate_items_impl: d / 64 > 8 unsupported
    TPW1_MAX_TARGETS=16 * 288,      # hgt_edge_agg_items.hip: tpw = NQ <= 16 * 288 ? 1 : 2
    RUNS_SHARED_MIN_DKP=32,         # hgt_edge_agg_items.hip launch_runs: shared relation transform from d_k 32 on ...
    RUNS_SHARED_MAX_ITEM=16,        # ... for items of <= 16 edges
    LOGITS_SHARED_MIN_DKP=64,       # hgt_edge_logits_mfma.hip launch_logits_mfma
    LOGITS_SHARED_MAX_ITEM=16,
    CH=512, MIN_ITEM=16,            # hgt_common.h HGT_CH / HGT_MIN_ITEM
    ITEM_MIN_COUNT=4096,            # hgt_common.h hgt_item_edges: E / ch < 4096 halves the item
    HUB_DEG=1024, TD=256,           # hgt_common.h HGT_HUB_DEG / HGT_TD
    SUB=16,                         # hgt_edge_common.h HGT_SUB
    SMALL_SUB=2,                    # hgt_edge_agg_mfma.hip HGT_SMALL_SUB
    SUB_FULL_NODES=65536,           # hgt_edge_agg_mfma.hip launch_agg_mfma: sub = NQ < 65536 ? (small ? HGT_SMALL_SUB : 4) : HGT_SUB
    SMALL_SUB_NODES=6144, SMALL_SUB_MAX_R=16, MID_SUB=4,
    VALU_SUB_FULL_NODES=65536, VALU_MID_SUB=4,      # hgt_edge_agg_valu.hip LaunchAggregate: sub = NQ < 65536 ? 4 : HGT_SUB
    KSIDE_MIN_ITEM=64,              # hgt_api.hip route(): hgt_edge_logits_kside by default from 64-edge work items on
    KSIDE_TABLE_LOG2=32,            # hgt_api.hip route(): ... with every Q / K row below 1 << 32 bytes from its base
    KSIDE_DK=32,                    # hgt_kside_map.h HGT_KSIDE_DK: the padded head width that kernel covers
    KSIDE_HEADS_A=2, KSIDE_HEADS_B=4, KSIDE_HEADS_C=8,      # hgt_edge_logits_kside.hip kside_layout: one head group of such heads
)

_SOURCE_PATTERNS = [
    # (file, regex, names of its groups)
    ("hgt_api.hip", r"#define HGT_FUSED_MIN_NODES (\d+)", ["FUSED_MIN_NODES"]),
    ("hgt_api.hip", r"#define HGT_ITEM_AGG_MAX_NODES (\d+)", ["ITEM_AGG_MAX_NODES"]),
    ("hgt_api.hip", r"#define HGT_ITEM_AGG_DEFAULT_NODES (\d+)", ["ITEM_AGG_DEFAULT_NODES"]),
    ("hgt_api.hip", r"if \(zb <= \(\(uint64_t\)1 << (\d+)\)\) w\.zitems_bytes = zb;", ["ITEM_SCRATCH_MAX_LOG2"]),
    ("hgt_api.hip", r"w\.zitems_bytes > 0 && NQ < HGT_ITEM_AGG_MAX_NODES && R < (\d+) &&", ["ITEM_MAX_RELATIONS"]),
    ("hgt_api.hip", r"const bool fused = split && !dense && dp <= (\d+) && dout <= dp &&", ["FUSED_MAX_DP"]),
    ("hgt_api.hip", r"HGT_FLAG_NO_MERGE_UPDATE\) && dp <= (\d+) && dout <= (\d+) && dout <= dp",
     ["MERGE_UPDATE_MAX_DP", "MERGE_UPDATE_MAX_DOUT"]),
    ("hgt_api.hip", r"fuse_update = !dense && split && \(dout <= (\d+) \|\| \(dout <= (\d+) && dp <= (\d+)\)\)",
     ["UPDATE_FUSED_DOUT", "UPDATE_WIDE_DOUT", "UPDATE_WIDE_DP"]),
    ("hgt_api.hip", r"stage != 4 && \(dkp >= (\d+) \|\| \(fl & HGT_FLAG_MFMA_LOGITS\)\)", ["MFMA_LOGITS_MIN_DKP"]),
    # (whole statements: _forward_route restates the covered set and the flag rule, so a term added or dropped is an error here)
    ("hgt_api.hip", r"const bool kside_covered = have_kside && split && !a->use_rte && stage != 4 &&\s*"
                    r"\(uint64_t\)N \* \(uint64_t\)H \* \(uint64_t\)dkp \* 4u < \(1ull << (\d+)\);", ["KSIDE_TABLE_LOG2"]),
    ("hgt_api.hip", r"const bool kside = kside_covered && !\(fl & HGT_FLAG_NO_KSIDE_LOGITS\) &&\s*"
                    r"\(\(fl & HGT_FLAG_KSIDE_LOGITS\) \|\| \(hgt_item_edges\(E\) >= (\d+) && "
                    r"!\(fl & \(HGT_FLAG_MFMA_LOGITS \| HGT_FLAG_VALU_LOGITS\)\)\)\);", ["KSIDE_MIN_ITEM"]),
    ("hgt_kside_map.h", r"constexpr int HGT_KSIDE_DK = (\d+);", ["KSIDE_DK"]),
    ("hgt_edge_logits_kside.hip", r"static bool kside_layout\(int32_t H, int32_t dk_pad\) \{ return dk_pad == HGT_KSIDE_DK && "
                                  r"\(H == (\d+) \|\| H == (\d+) \|\| H == (\d+)\); \}", ["KSIDE_HEADS_A", "KSIDE_HEADS_B", "KSIDE_HEADS_C"]),
    ("hgt_edge_agg_items.hip", r"R >= (\d+) \|\| d % 64 != 0 \|\| d / 64 > (\d+)\) return HGT_ERR_UNSUPPORTED", [None, "ITEM_MAX_VF"]),
    ("hgt_edge_agg_items.hip", r"const int tpw = NQ <= ([\d *+]+) \? 1 : 2;", ["TPW1_MAX_TARGETS"]),
    ("hgt_edge_agg_items.hip", r"if constexpr \(G::DKP >= (\d+) && G::NCT % 4 == 0 && \(G::NCT / 4\) \* G::NKS <= 8\) \{\s*"
                               r"if \(!\(mode & 2\) && \(\(mode & 4\) \|\| item_edges <= (\d+)\)\)",
     ["RUNS_SHARED_MIN_DKP", "RUNS_SHARED_MAX_ITEM"]),
    ("hgt_edge_logits_mfma.hip", r"if constexpr \(G::DKP >= (\d+) && G::NCT % 4 == 0 && \(G::NCT / 4\) \* G::NKS <= 8\) \{\s*"
                                 r"if \(!\(mode & 2\) && \(\(mode & 4\) \|\| item_edges <= (\d+)\)\)",
     ["LOGITS_SHARED_MIN_DKP", "LOGITS_SHARED_MAX_ITEM"]),
    ("hgt_common.h", r"#define HGT_CH (\d+)", ["CH"]),
    ("hgt_common.h", r"#define HGT_MIN_ITEM (\d+)", ["MIN_ITEM"]),
    ("hgt_common.h", r"while \(ch > HGT_MIN_ITEM && E / ch < (\d+)\) ch >>= 1;", ["ITEM_MIN_COUNT"]),
    ("hgt_common.h", r"#define HGT_HUB_DEG (\d+)", ["HUB_DEG"]),
    ("hgt_common.h", r"#define HGT_TD (\d+)", ["TD"]),
    ("hgt_edge_common.h", r"constexpr int HGT_SUB = (\d+);", ["SUB"]),
    ("hgt_edge_agg_mfma.hip", r"#define HGT_SMALL_SUB (\d+)", ["SMALL_SUB"]),
    ("hgt_edge_agg_mfma.hip", r"const int sub = \(NQ < (\d+)\) \? \(\(NQ < (\d+) && ny_ == 1 && R <= (\d+)\) \? HGT_SMALL_SUB : (\d+)\) : HGT_SUB;",
     ["SUB_FULL_NODES", "SMALL_SUB_NODES", "SMALL_SUB_MAX_R", "MID_SUB"]),
    ("hgt_edge_agg_valu.hip", r"const int sub = \(NQ < (\d+)\) \? (\d+) : HGT_SUB;", ["VALU_SUB_FULL_NODES", "VALU_MID_SUB"]),
]
_SOURCE_CACHE = {}


def _int_expr(text):
    """A sum of products of integer literals, as the sources write some thresholds (16 * 288)."""
    total = 0
    for term in text.split("+"):
        prod = 1
        for factor in term.split("*"):
            prod *= int(factor)
        total += prod
    return total


def _source_constants():
    """The constants of the route as the sources state them today.  A line that no longer matches its pattern is an error: the
    restated route below has to be revisited together with it."""
    if not _SOURCE_CACHE:
        text, consts = {}, {}
        for fname, pat, names in _SOURCE_PATTERNS:
            if fname not in text:
                with open(os.path.join(CSRC, fname)) as f:
                    text[fname] = f.read()
            found = re.findall(pat, text[fname])
            assert len(found) == 1, "%s: expected exactly one match of %r, found %d" % (fname, pat, len(found))
            vals = found[0] if isinstance(found[0], tuple) else (found[0],)
            for name, v in zip(names, vals):
                if name is not None:
                    consts[name] = _int_expr(v)
        _SOURCE_CACHE.update(consts)          # (only a complete set: every test that needs it repeats the error of a line that moved)
    return dict(_SOURCE_CACHE)


# ------------------------------------------------------------------ 1. the route, restated
def _layout(d, n_heads):
    """hgt_layout_compute (hgt_common.h): heads rounded up to a power of two, d_k padded to vec * lanes per head."""
    heads = 1
    while heads < n_heads:
        heads *= 2
    dk, lph, vec = d // n_heads, 64 // heads, 1
    while vec * lph < dk:
        vec *= 2
    assert vec <= 16 and lph >= 4, "hgt_layout_for refuses this shape"
    return dict(heads=heads, dk=dk, lph=lph, vec=vec, dkp=vec * lph, dp=64 * vec)


def _mfma_split(vec_full, lph):
    """mfma_split_for (hgt_edge_common.h): head groups per row so that a wavefront's slice is <= 256 columns; 0 = not covered."""
    s = 1
    while vec_full // s > 4 and lph * s * 2 <= 64:
        s *= 2
    return s if vec_full // s <= 4 else 0


def _item_edges(E, K):
    """hgt_item_edges (hgt_common.h)."""
    ch = K["CH"]
    while ch > K["MIN_ITEM"] and E // ch < K["ITEM_MIN_COUNT"]:
        ch >>= 1
    return ch


def _align(v, a=256):
    return (v + a - 1) // a * a


def _item_scratch_bytes(E, heads, dkp):
    """hgt_edge_aggregate_items_bytes: [E][d] transformed rows | [E][H][2] run statistics | [E] run-start flags."""
    return _align(E * heads * dkp * 4) + _align(E * heads * 8) + _align(E)


def _scratch_gate_edges(heads, dkp, K):
    """The largest E whose item-parallel scratch passes conv_workspace's gate (the byte count never decreases with E)."""
    gate, lo, hi = 1 << K["ITEM_SCRATCH_MAX_LOG2"], 0, 1 << 31
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if _item_scratch_bytes(mid, heads, dkp) <= gate else (lo, mid - 1)
    return lo


def _shared_transform(vec, lph, item_edges, min_dkp, max_item, flags):
    """The `if constexpr (G::DKP >= .. && G::NCT % 4 == 0 && (G::NCT / 4) * G::NKS <= 8)` + item length test of launch_logits_mfma and
    launch_runs: the relation transform is shared by the four wavefronts of a workgroup."""
    dkp, nct = vec * lph, 64 * vec // 16
    nks = max(dkp, 32) // 32
    if not (dkp >= min_dkp and nct % 4 == 0 and (nct // 4) * nks <= 8):
        return False
    return not (flags & _lib.HGT_FLAG_NO_COOP_EDGE) and bool((flags & _lib.HGT_FLAG_COOP_EDGE_ALWAYS) or item_edges <= max_item)


LOGITS_MFMA_LAYOUTS = {(4, 8), (4, 16), (4, 32), (4, 64), (2, 32), (2, 64), (1, 64)}      # hgt_launch_logits_mfma: LGM_CASE


def _forward_route(N, NQ, E, d, H, R, precision, dense=False, flags=0, item_scratch=None, K=None, use_rte=False):
    """What Conv::route() and the kernels' own dispatch decide for a whole-layer call (stage 0, in_dim == out_dim == d, d % 4 == 0,
    hubs possible).  use_rte: the layer has a temporal encoding (only the logits kernel depends on it).  item_scratch: the workspace holds the item-parallel scratch if the library grants it -- None: what
    HGTConv.forward asks for with its own workspace (split precision and no HGT_FLAG_NO_ITEM_AGGREGATE); False: a caller-owned
    workspace of workspace_bytes(staged=True).  Returns the forms that ANSWER (a form that returns HGT_ERR_UNSUPPORTED hands over
    to the next one; `tried` lists them in order)."""
    K = K or _source_constants()
    F = _lib
    L = _layout(d, H)
    dp, dkp, lph, heads = L["dp"], L["dkp"], L["lph"], L["heads"]
    split, f16 = precision != "fp32", precision == "f16x3"
    if item_scratch is None:
        item_scratch = split and not (flags & F.HGT_FLAG_NO_ITEM_AGGREGATE)
    sp = _mfma_split(dkp // lph, lph)
    vec_s, lph_s = (dkp // lph // sp, lph * sp) if sp else (0, 0)
    have_frags = split and sp != 0                                  # hgt_relation_frag_bytes > 0
    mfma_agg = have_frags and not (flags & F.HGT_FLAG_VALU_AGGREGATE)
    ie = _item_edges(E, K)
    r = dict(item_edges=ie, qkv_launches=1 if NQ == N else 2, dp=dp, dkp=dkp)
    # logits
    mfma_logits = have_frags and not (flags & F.HGT_FLAG_VALU_LOGITS) and (dkp >= K["MFMA_LOGITS_MIN_DKP"] or bool(flags & F.HGT_FLAG_MFMA_LOGITS))
    mfma_logits = mfma_logits and (vec_s, lph_s) in LOGITS_MFMA_LAYOUTS         # (else hgt_launch_logits_mfma hands over)
    # ... on the source side, per edge (hgt_edge_logits_kside), where that kernel is covered and, by default, the items are long enough
    kside_covered = (split and dkp == K["KSIDE_DK"] and heads in (K["KSIDE_HEADS_A"], K["KSIDE_HEADS_B"], K["KSIDE_HEADS_C"]) and
                     not use_rte and N * heads * dkp * 4 < (1 << K["KSIDE_TABLE_LOG2"]))
    kside = (kside_covered and not (flags & F.HGT_FLAG_NO_KSIDE_LOGITS) and
             (bool(flags & F.HGT_FLAG_KSIDE_LOGITS) or
              (ie >= K["KSIDE_MIN_ITEM"] and not (flags & (F.HGT_FLAG_MFMA_LOGITS | F.HGT_FLAG_VALU_LOGITS)))))
    r["kside_covered"] = kside_covered
    r["logits"] = "kside" if kside else "mfma" if mfma_logits else "valu"
    r["logits_shared"] = mfma_logits and not kside and _shared_transform(vec_s, lph_s, ie, K["LOGITS_SHARED_MIN_DKP"], K["LOGITS_SHARED_MAX_ITEM"], flags)
    # the scratch of the item-parallel form: sized from N (conv_workspace), part of the workspace only if the caller sized it in
    scratch = _item_scratch_bytes(E, heads, dkp)
    r["item_scratch_bytes"] = scratch
    zitems = bool(item_scratch) and N < K["ITEM_AGG_MAX_NODES"] and scratch <= (1 << K["ITEM_SCRATCH_MAX_LOG2"])
    r["item_scratch_granted"] = zitems
    fused = (split and not dense and dp <= K["FUSED_MAX_DP"] and d <= dp and
             (NQ >= K["FUSED_MIN_NODES"] or bool(flags & F.HGT_FLAG_FUSED_ANY_SIZE)) and not (flags & F.HGT_FLAG_NO_FUSED_UPDATE) and
             not (f16 and not mfma_agg))
    items = (mfma_agg and zitems and NQ < K["ITEM_AGG_MAX_NODES"] and R < K["ITEM_MAX_RELATIONS"] and
             not (flags & F.HGT_FLAG_NO_ITEM_AGGREGATE) and (NQ < K["ITEM_AGG_DEFAULT_NODES"] or bool(flags & F.HGT_FLAG_ITEM_AGGREGATE)))
    order = []
    if fused:
        order.append("fused")
    if items and not dense and not (flags & F.HGT_FLAG_NO_MERGE_UPDATE) and dp <= K["MERGE_UPDATE_MAX_DP"] and d <= K["MERGE_UPDATE_MAX_DOUT"] and d <= dp:
        order.append("items_update")
    if items:
        order.append("items")
    order.append("subtile")
    tried = []
    for form in order:
        tried.append(form)
        if form == "fused":
            # matrix cores: no head-group split (true for dp <= 256) and the R + 1 ranges in lane registers; vector ALU otherwise
            if (mfma_agg and sp == 1 and R < 64) or not mfma_agg:
                break
        elif form in ("items_update", "items"):
            if dp // 64 <= K["ITEM_MAX_VF"] and sp != 0:      # aggregate_items_impl: d / 64 > 8 -> HGT_ERR_UNSUPPORTED
                break
        else:
            break
    agg = tried[-1]
    r.update(tried=tried, agg=agg, tpw=None, sub=None, agg_kernel=None, runs_shared=None)
    if agg in ("items_update", "items"):
        r["runs_shared"] = _shared_transform(vec_s, lph_s, ie, K["RUNS_SHARED_MIN_DKP"], K["RUNS_SHARED_MAX_ITEM"], flags)
    if agg == "items_update":
        r["tpw"] = 1 if NQ <= K["TPW1_MAX_TARGETS"] else 2
    if agg == "fused":          # (64 targets per workgroup, HGT_SUB per wavefront whatever NQ: the fused kernels have no `sub`)
        r["agg_kernel"] = "mfma" if mfma_agg else "valu"
    if agg == "subtile":
        if mfma_agg:            # launch_agg_mfma; ny = head groups of the row
            small = NQ < K["SMALL_SUB_NODES"] and sp == 1 and R <= K["SMALL_SUB_MAX_R"]
            r.update(agg_kernel="mfma", sub=(K["SMALL_SUB"] if small else K["MID_SUB"]) if NQ < K["SUB_FULL_NODES"] else K["SUB"])
        else:                   # hgt_valu_aggregate
            r.update(agg_kernel="valu", sub=K["VALU_MID_SUB"] if NQ < K["VALU_SUB_FULL_NODES"] else K["SUB"])
    fuse_update = not dense and split and (d <= K["UPDATE_FUSED_DOUT"] or (d <= K["UPDATE_WIDE_DOUT"] and dp <= K["UPDATE_WIDE_DP"]))
    r["update"] = ("in_aggregation" if agg in ("fused", "items_update") else
                   "dense" if dense else "linear_fused" if fuse_update else "linear_node")
    return r


def _forcing_flags(agg):
    """The flags that put `agg` first wherever the library can run it at all."""
    F = _lib
    return {"fused": F.HGT_FLAG_FUSED_ANY_SIZE,
            "items_update": F.HGT_FLAG_ITEM_AGGREGATE | F.HGT_FLAG_NO_FUSED_UPDATE,
            "items": F.HGT_FLAG_ITEM_AGGREGATE | F.HGT_FLAG_NO_FUSED_UPDATE | F.HGT_FLAG_NO_MERGE_UPDATE,
            "subtile": F.HGT_FLAG_NO_ITEM_AGGREGATE | F.HGT_FLAG_NO_FUSED_UPDATE}[agg]


def test_restated_constants_match_the_sources():
    K = _source_constants()
    assert K == RESTATED, {k: (K.get(k), RESTATED.get(k)) for k in set(K) | set(RESTATED) if K.get(k) != RESTATED.get(k)}


FL = _lib
HAND_ROWS = [
    # (N, NQ, E, d, H, R, precision, dense, flags, item_scratch) -> the entries of the route derived by hand from the sources
    ((4608, 4608, 46080, 256, 8, 8, "bf16x3", False, 0, None),
     dict(logits="valu", agg="items_update", tpw=1, item_edges=16, runs_shared=True, update="in_aggregation", qkv_launches=1)),
    ((4609, 4609, 46090, 256, 8, 8, "f16x3", False, 0, None), dict(agg="items_update", tpw=2)),
    ((16383, 16383, 163830, 64, 4, 4, "bf16x3", False, 0, None),
     dict(logits="valu", agg="items_update", tpw=2, item_edges=32, runs_shared=False, dp=64, dkp=16)),
    ((16384, 16384, 163840, 256, 8, 8, "bf16x3", False, 0, None),
     dict(agg="fused", agg_kernel="mfma", tried=["fused"], sub=None, tpw=None, update="in_aggregation", item_edges=32)),
    ((16384, 16384, 163840, 512, 8, 9, "f16x3", False, 0, None),
     dict(logits="mfma", logits_shared=False, agg="items_update", tpw=2, tried=["items_update"], dp=512, dkp=64)),
    ((3000, 3000, 30000, 512, 8, 9, "f16x3", False, 0, None), dict(logits="mfma", logits_shared=True, agg="items_update", tpw=1)),
    ((16384, 16384, 163840, 400, 8, 9, "bf16x3", False, 0, None), dict(dp=512, dkp=64, agg="items_update", update="in_aggregation")),
    # n_hid 768 is 1024 padded columns: the scratch of 10 edges per node is 2.7 GB (gate), a smaller E gets it and the kernel refuses
    ((65536, 65536, 655360, 768, 8, 5, "f16x3", False, 0, None),
     dict(dp=1024, dkp=128, logits="mfma", logits_shared=False, tried=["subtile"], agg_kernel="mfma", sub=16, update="linear_node",
          item_edges=128, item_scratch_granted=False)),
    ((65535, 65535, 655350, 768, 8, 5, "f16x3", False, 0, None), dict(tried=["subtile"], sub=4, item_scratch_granted=False)),
    ((65535, 65535, 250000, 768, 8, 5, "bf16x3", False, 0, None),
     dict(tried=["items", "subtile"], agg="subtile", sub=4, update="linear_node", item_edges=32, item_scratch_granted=True)),
    ((65535, 65535, 655350, 64, 4, 4, "fp32", False, 0, None),
     dict(logits="valu", tried=["subtile"], agg_kernel="valu", sub=4, update="linear_node", item_scratch_granted=False)),
    ((65536, 65536, 655360, 64, 4, 4, "fp32", False, 0, None), dict(agg_kernel="valu", sub=16, update="linear_node")),
    ((65535, 65535, 655350, 256, 8, 8, "bf16x3", False, 0, None), dict(agg="fused", item_scratch_granted=True)),
    ((65536, 65536, 655360, 256, 8, 8, "bf16x3", False, 0, None), dict(agg="fused", item_scratch_granted=False)),
    ((20000, 20000, 200000, 256, 8, 8, "bf16x3", True, 0, None), dict(tried=["items"], agg="items", update="dense", runs_shared=False)),
    ((66000, 66000, 660000, 400, 8, 8, "f16x3", True, 0, None), dict(tried=["subtile"], agg_kernel="mfma", sub=16, update="dense")),
    ((70000, 10000, 100000, 256, 8, 8, "bf16x3", False, 0, None),
     dict(tried=["subtile"], sub=4, update="linear_fused", qkv_launches=2, item_scratch_granted=False)),
    ((60000, 10000, 100000, 256, 8, 8, "bf16x3", False, 0, None), dict(agg="items_update", tpw=2, qkv_launches=2)),
    ((6143, 6143, 61430, 256, 8, 16, "bf16x3", False, 0, False), dict(tried=["subtile"], sub=2, update="linear_fused")),
    ((6143, 6143, 61430, 256, 8, 17, "bf16x3", False, 0, False), dict(sub=4)),
    ((6144, 6144, 61440, 256, 8, 16, "bf16x3", False, 0, False), dict(sub=4)),
    ((6143, 6143, 61430, 512, 8, 16, "bf16x3", False, 0, False), dict(sub=4, update="linear_fused")),      # two head groups
    ((3000, 3000, 30000, 256, 8, 63, "bf16x3", False, 0, None), dict(agg="items_update", tpw=1)),
    ((3000, 3000, 30000, 256, 8, 64, "bf16x3", False, 0, None), dict(tried=["subtile"], sub=4, update="linear_fused")),
    # 1089 bytes per edge at d = 256 / 8 heads: 1088 * 985 988 + align(985 988, 256) = 2^30 - 768; one edge more is 2^30 + 512 (its [E][8][2] statistics need padding)
    ((12000, 12000, 985988, 256, 8, 8, "bf16x3", False, 0, None), dict(agg="items_update", item_scratch_bytes=(1 << 30) - 768, item_edges=128)),
    ((12000, 12000, 985989, 256, 8, 8, "bf16x3", False, 0, None),
     dict(tried=["subtile"], sub=4, update="linear_fused", item_scratch_bytes=(1 << 30) + 512)),
    ((12000, 12000, 131071, 64, 4, 4, "bf16x3", False, 0, None), dict(item_edges=16, item_scratch_bytes=37879552)),      # 289 B per edge
    ((12000, 12000, 131072, 64, 4, 4, "bf16x3", False, 0, None), dict(item_edges=32)),
    ((12000, 12000, 2097151, 64, 4, 4, "bf16x3", False, 0, None), dict(item_edges=256, agg="items_update")),
    ((60000, 60000, 2097152, 64, 4, 4, "bf16x3", False, 0, None), dict(item_edges=512, agg="fused", logits="valu")),
    # flags
    ((3000, 3000, 30000, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_FUSED_ANY_SIZE, None), dict(agg="fused")),
    ((20000, 20000, 200000, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_NO_FUSED_UPDATE, None), dict(agg="items_update", tpw=2)),
    ((20000, 20000, 200000, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_NO_FUSED_UPDATE | FL.HGT_FLAG_NO_MERGE_UPDATE, None),
     dict(agg="items", update="linear_fused")),
    ((20000, 20000, 200000, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_NO_FUSED_UPDATE | FL.HGT_FLAG_NO_ITEM_AGGREGATE, None),
     dict(tried=["subtile"], sub=4, update="linear_fused")),
    ((3000, 3000, 30000, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_MFMA_LOGITS, None), dict(logits="mfma", logits_shared=False)),
    # one head of 512 columns: no matrix-core edge kernel covers it (mfma_split_for == 0)
    ((3000, 3000, 30000, 512, 1, 4, "bf16x3", False, 0, None), dict(logits="valu", tried=["subtile"], agg_kernel="valu", sub=4, update="linear_fused")),
    # the K-side logits kernel (an eleventh entry: use_rte).  hgt_item_edges(262 144) = 64 is its default line at 32-column heads
    ((12000, 12000, 262143, 256, 8, 8, "bf16x3", False, 0, None), dict(logits="valu", kside_covered=True, item_edges=32, dkp=32)),
    ((12000, 12000, 262144, 256, 8, 8, "bf16x3", False, 0, None), dict(logits="kside", kside_covered=True, item_edges=64, logits_shared=False)),
    ((12000, 12000, 262144, 256, 8, 8, "f16x3", False, 0, None), dict(logits="kside", item_edges=64)),
    ((12000, 12000, 262143, 256, 8, 8, "bf16x3", False, 0, None, True), dict(logits="valu", kside_covered=False, item_edges=32)),
    ((12000, 12000, 262144, 256, 8, 8, "bf16x3", False, 0, None, True), dict(logits="valu", kside_covered=False, item_edges=64)),
    ((12000, 12000, 262143, 256, 8, 8, "fp32", False, 0, None), dict(logits="valu", kside_covered=False)),
    ((12000, 12000, 262144, 256, 8, 8, "fp32", False, 0, None), dict(logits="valu", kside_covered=False, item_edges=64)),
    ((12000, 12000, 262144, 512, 16, 8, "bf16x3", False, 0, None), dict(logits="valu", kside_covered=False, dkp=32, dp=512)),      # 16 heads
    ((12000, 12000, 262144, 128, 8, 8, "bf16x3", False, 0, None), dict(logits="valu", kside_covered=False, dkp=16)),
    ((12000, 12000, 262144, 512, 8, 9, "bf16x3", False, 0, None), dict(logits="mfma", kside_covered=False, dkp=64)),
    ((12000, 12000, 262144, 96, 3, 8, "bf16x3", False, 0, None), dict(logits="kside", kside_covered=True, dkp=32, dp=128)),          # 3 heads run as 4
    ((12000, 12000, 262144, 64, 2, 8, "f16x3", False, 0, None), dict(logits="kside", dkp=32, dp=64)),
    ((12000, 12000, 262144, 128, 4, 8, "f16x3", False, 0, None), dict(logits="kside", dkp=32, dp=128)),
    # rows of 1024 bytes: node 4 194 304 would start 4 GiB from the base (route rows only: nothing this large is allocated)
    ((4194303, 4194303, 41943030, 256, 8, 8, "bf16x3", False, 0, None), dict(logits="kside", kside_covered=True, item_edges=512)),
    ((4194304, 4194304, 41943040, 256, 8, 8, "bf16x3", False, 0, None), dict(logits="valu", kside_covered=False, item_edges=512)),
    ((3000, 3000, 30000, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_KSIDE_LOGITS, None), dict(logits="kside", item_edges=16)),
    ((3000, 3000, 30000, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_KSIDE_LOGITS | FL.HGT_FLAG_VALU_LOGITS, None), dict(logits="kside")),
    ((3000, 3000, 30000, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_KSIDE_LOGITS | FL.HGT_FLAG_MFMA_LOGITS, None), dict(logits="kside", logits_shared=False)),
    ((3000, 3000, 30000, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_KSIDE_LOGITS, None, True), dict(logits="valu")),
    ((3000, 3000, 30000, 256, 8, 8, "fp32", False, FL.HGT_FLAG_KSIDE_LOGITS, None), dict(logits="valu")),
    ((12000, 12000, 262144, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_MFMA_LOGITS, None), dict(logits="mfma", item_edges=64)),
    ((12000, 12000, 262144, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_VALU_LOGITS, None), dict(logits="valu")),
    ((12000, 12000, 262144, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_NO_KSIDE_LOGITS, None), dict(logits="valu", kside_covered=True)),
    ((12000, 12000, 262144, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_NO_KSIDE_LOGITS | FL.HGT_FLAG_KSIDE_LOGITS, None), dict(logits="valu")),
    ((12000, 12000, 262144, 256, 8, 8, "bf16x3", False, FL.HGT_FLAG_NO_KSIDE_LOGITS | FL.HGT_FLAG_MFMA_LOGITS, None), dict(logits="mfma")),
]


def _hand_row_id(a):
    return "%d-%d-%d-d%d-h%d-r%d-%s-%s-f%d-%s" % a[:10] + ("-rte" if len(a) > 10 and a[10] else "")


@pytest.mark.parametrize("args,expect", HAND_ROWS, ids=[_hand_row_id(a) for a, _ in HAND_ROWS])
def test_forward_route_against_hand_derived_rows(args, expect):
    r = _forward_route(*args[:10], use_rte=len(args) > 10 and args[10])
    for k, v in expect.items():
        assert r[k] == v, (k, r)


def test_scratch_gate_edges_is_the_last_count_that_passes():
    K = _source_constants()
    for heads, dkp, want in ((8, 32, 985988), (8, 64, None), (4, 16, None)):
        e = _scratch_gate_edges(heads, dkp, K)
        assert _item_scratch_bytes(e, heads, dkp) <= 1 << 30 < _item_scratch_bytes(e + 1, heads, dkp)
        assert want is None or e == want


# ------------------------------------------------------------------ 2. the cases
def _case(cid, N, d, H, expect, NQ=None, E=None, T=4, R=8, line=None, dense=False, precisions=("bf16x3", "f16x3"), own_ws=False):
    return dict(id=cid, N=N, NQ=N if NQ is None else NQ, E=E, d=d, H=H, T=T, R=R, expect=expect, line=line, dense=dense,
                precisions=precisions, own_ws=own_ws)


def _build_cases():
    K = RESTATED
    HEADS = {64: 4, 256: 8, 400: 8, 512: 8, 768: 8}
    cs = []
    # two targets per wavefront of the merge+update kernel: 16 * 288 = 4608 is the last size with one; 16 383 the last unfused size
    for d in (64, 256, 400, 512):
        for nq, tpw in ((4608, 1), (4609, 2), (16383, 2)):
            cs.append(_case("tpw-%d-d%d" % (nq, d), nq, d, HEADS[d], dict(agg="items_update", tpw=tpw, update="in_aggregation"),
                            line=4608 if nq < 5000 else 16384, R=9 if d >= 400 else 8))
    # the fused line (16 383 at d = 64 / 256 is in the list above)
    cs.append(_case("fused-16384-d256", 16384, 256, 8, dict(agg="fused", agg_kernel="mfma", tried=["fused"]), line=16384))
    cs.append(_case("fused-16384-d64", 16384, 64, 4, dict(agg="fused", agg_kernel="mfma", tried=["fused"]), line=16384, T=3, R=4))
    cs.append(_case("fused-16384-d512", 16384, 512, 8, dict(agg="items_update", tpw=2, tried=["items_update"], logits="mfma"), line=16384, R=9))
    # the 65 536 line
    cs.append(_case("n65535-d256", 65535, 256, 8, dict(agg="fused", item_scratch_granted=True, logits="kside"), line=65536))
    cs.append(_case("n65536-d256", 65536, 256, 8, dict(agg="fused", item_scratch_granted=False, logits="valu"), line=65536))      # (temporal)
    cs.append(_case("n65535-d768", 65535, 768, 8, dict(tried=["subtile"], agg_kernel="mfma", sub=4, update="linear_node", dp=1024),
                    line=65536, T=3, R=5))
    cs.append(_case("n65536-d768", 65536, 768, 8, dict(tried=["subtile"], agg_kernel="mfma", sub=16, update="linear_node", dp=1024),
                    line=65536, T=3, R=5))
    # (10 edges per node make 2.7 GB of scratch at 1024 columns, which the gate refuses before the kernel is asked; with 250 000
    #  edges the scratch is granted, the item-parallel form answers HGT_ERR_UNSUPPORTED and the sub-tile kernel takes over)
    cs.append(_case("n65535-d768-e250000", 65535, 768, 8, dict(tried=["items", "subtile"], sub=4, update="linear_node", item_scratch_granted=True),
                    E=250000, line=65536, T=3, R=5))
    # edges per work item: the doubling points of hgt_item_edges
    for i, e in enumerate((131072, 262144, 524288, 1048576, 2097152)):
        for ee, ie in ((e - 1, 16 << i), (e, 32 << i)):
            cs.append(_case("items-n12000-e%d" % ee, 12000, 64, 4, dict(agg="items_update", tpw=2, item_edges=ie, logits="valu"), E=ee, T=3, R=4))
    for ee, ie in ((2097151, 256), (2097152, 512)):
        cs.append(_case("items-n60000-e%d" % ee, 60000, 64, 4, dict(agg="fused", item_edges=ie, logits="valu"), E=ee, T=3, R=4))
    # the item-parallel form switched off without a flag
    for d in (256, 512):
        L = _layout(d, 8)
        e = _scratch_gate_edges(L["heads"], L["dkp"], K)
        cs.append(_case("gate-under-d%d" % d, 12000, d, 8, dict(agg="items_update", tpw=2, item_scratch_granted=True, logits="valu" if d == 256 else "mfma"), E=e, R=9 if d == 512 else 8))      # (temporal)
        cs.append(_case("gate-over-d%d" % d, 12000, d, 8, dict(tried=["subtile"], agg_kernel="mfma", sub=4, update="linear_fused",
                                                              item_scratch_granted=False, logits="kside" if d == 256 else "mfma"),
                        E=e + 1, R=9 if d == 512 else 8))
    cs.append(_case("r63-n3000", 3000, 256, 8, dict(agg="items_update", tpw=1), T=3, R=63))
    cs.append(_case("r64-n3000", 3000, 256, 8, dict(tried=["subtile"], agg_kernel="mfma", sub=4, update="linear_fused"), T=3, R=64))
    cs.append(_case("halo-n60000-q10000", 60000, 256, 8, dict(agg="items_update", tpw=2, qkv_launches=2, item_scratch_granted=True), NQ=10000))
    cs.append(_case("halo-n70000-q10000", 70000, 256, 8, dict(tried=["subtile"], agg_kernel="mfma", sub=4, update="linear_fused", qkv_launches=2,
                                                             item_scratch_granted=False), NQ=10000))
    for nq, rr, sub in ((6143, 16, 2), (6144, 16, 4), (6143, 17, 4), (6144, 17, 4)):
        cs.append(_case("ownws-%d-r%d" % (nq, rr), nq, 256, 8, dict(tried=["subtile"], agg_kernel="mfma", sub=sub, update="linear_fused",
                                                                   item_scratch_granted=False), R=rr, line=6144, own_ws=True))
    # halo rows at fused sizes
    cs.append(_case("halo-n40000-q16383", 40000, 256, 8, dict(agg="items_update", tpw=2, qkv_launches=2), NQ=16383, line=16384))
    cs.append(_case("halo-n40000-q16384", 40000, 256, 8, dict(agg="fused", qkv_launches=2), NQ=16384, line=16384))
    # DenseHGTConv
    for d in (256, 400):
        cs.append(_case("dense-n20000-d%d" % d, 20000, d, 8, dict(tried=["items"], update="dense", logits="valu" if d == 256 else "mfma"),
                        dense=True, T=5 if d == 400 else 4, R=9))      # (temporal)
        cs.append(_case("dense-n66000-d%d" % d, 66000, d, 8, dict(tried=["subtile"], agg_kernel="mfma", sub=16, update="dense",
                                                                 logits="kside" if d == 256 else "mfma"), dense=True, T=5 if d == 400 else 4, R=9))
    # exact fp32: the vector-ALU sub-tile kernel has the same 65 536 line
    cs.append(_case("fp32-n65535-d64", 65535, 64, 4, dict(tried=["subtile"], agg_kernel="valu", sub=4, update="linear_node"), line=65536,
                    T=3, R=4, precisions=("fp32",)))
    cs.append(_case("fp32-n65536-d64", 65536, 64, 4, dict(tried=["subtile"], agg_kernel="valu", sub=16, update="linear_node"), line=65536,
                    T=3, R=4, precisions=("fp32",)))
    for i, c in enumerate(cs):
        if c["E"] is None:
            c["E"] = 10 * c["NQ"]               # about ten in-edges per target
        c["use_norm"], c["use_rte"], c["keep_att"], c["strided"] = i % 3 != 1, i % 2 == 0, i % 3 == 0 or c["line"] in (16384, 65536), i % 2 == 1
    # The lines of the K-side logits kernel (hgt_edge_logits_kside), appended behind the loop so that the index-derived switches of the
    # cases above stay what they were: 64-edge items (E = 262 144) at every head count it covers, and what it does not cover.  Every
    # one keeps the attention weights: the GPU test reads the logits kernel off their bits.
    n_old = len(cs)
    ks = dict(E=262144, T=3, R=4)
    cs.append(_case("kside-e262143-d256", 12000, 256, 8, dict(logits="valu", kside_covered=True, item_edges=32), E=262143, T=3, R=4))
    cs.append(_case("kside-e262144-d256", 12000, 256, 8, dict(logits="kside", item_edges=64), **ks))
    cs.append(_case("kside-e262144-d256-rte", 12000, 256, 8, dict(logits="valu", kside_covered=False, item_edges=64), **ks))
    cs.append(_case("kside-e262144-d64-h2", 12000, 64, 2, dict(logits="kside", item_edges=64, dkp=32), **ks))
    cs.append(_case("kside-e262144-d128-h4", 12000, 128, 4, dict(logits="kside", item_edges=64, dkp=32), **ks))
    cs.append(_case("kside-e262144-d96-h3", 12000, 96, 3, dict(logits="kside", item_edges=64, dkp=32), **ks))
    cs.append(_case("kside-e262144-d128-h8", 12000, 128, 8, dict(logits="valu", kside_covered=False, item_edges=64, dkp=16), **ks))
    cs.append(_case("kside-e262144-d256-fp32", 12000, 256, 8, dict(logits="valu", kside_covered=False, item_edges=64), precisions=("fp32",), **ks))
    for i, c in enumerate(cs[n_old:]):
        c["use_norm"], c["use_rte"], c["keep_att"], c["strided"], c["logits_bits"] = i % 3 != 1, c["id"].endswith("-rte"), True, i % 2 == 1, True
    return cs


CASES = _build_cases()
CASE_PARAMS = [pytest.param(c, p, id="%s-%s" % (c["id"], p)) for c in CASES for p in c["precisions"]]


def _case_route(c, precision, flags=0):
    return _forward_route(c["N"], c["NQ"], c["E"], c["d"], c["H"], c["R"], precision, c["dense"], flags, False if c["own_ws"] else None,
                          use_rte=c["use_rte"])


@pytest.mark.parametrize("c,precision", CASE_PARAMS)
def test_every_case_sits_on_the_side_it_names(c, precision):
    """No GPU needed: with the constants of today's sources the case takes the route it was written for, and the flags that force
    that form reproduce it (the bit comparison of the GPU test is then between the same kernels)."""
    r = _case_route(c, precision)
    for k, v in c["expect"].items():
        assert r[k] == v, (c["id"], k, r)
    if precision != "fp32":
        f = _case_route(c, precision, _forcing_flags(r["agg"]))
        for k in ("agg", "update", "tpw", "sub", "agg_kernel", "logits", "item_edges"):
            assert f[k] == r[k], (c["id"], k, r, f)


def _graph(c, seed):
    """~E/NQ in-edges per target on the device: uniform sources over all N rows, targets over the first NQ; one hub target above
    HGT_HUB_DEG, every 17th edge of a relation id nobody claims, every 37th node (from node 5) of no known type."""
    N, NQ, E, d, T, R = c["N"], c["NQ"], c["E"], c["d"], c["T"], c["R"]
    g = torch.Generator(device=DEV).manual_seed(seed)
    nt_clean = torch.randint(0, T, (N,), generator=g, device=DEV).sort().values
    x = torch.randn(N, d, generator=g, device=DEV)
    src = torch.randint(0, N, (E,), generator=g, device=DEV)
    dst = torch.randint(0, NQ, (E,), generator=g, device=DEV)
    hub = NQ // 3 + 17
    n_hub = RESTATED["HUB_DEG"] + 476 + 4 * (E // NQ)
    dst[:n_hub] = hub
    et = torch.randint(0, R, (E,), generator=g, device=DEV)
    et[::17] = R + 2
    tm = torch.randint(0, 240, (E,), generator=g, device=DEV)
    nt = nt_clean.clone()
    nt[5::37] = T + 1
    ei = torch.stack([src, dst], dim=1).contiguous().t() if c["strided"] else torch.stack([src, dst], dim=0).contiguous()
    return dict(T=T, R=R, H=c["H"], d=d, N=N, NQ=NQ, E=E, x=x, nt=nt, nt_clean=nt_clean, ei=ei, et=et, tm=tm, hub=hub,
                use_rte=c["use_rte"], use_norm=c["use_norm"], ids=torch.arange(N, device=DEV).unsqueeze(1),
                deg=torch.bincount(dst, minlength=N))


def _fp64_rows_att(sd, g, targets, dense, att, max_edges=1 << 21):
    """_fp64_rows of test_hgt_gpu.py for DenseHGTConv too, and with the attention weights: returns (float64 rows, the largest
    |att - closed form| over ALL in-edges of the rows, their number).  The in-edges of a group of rows are taken in their original
    order (induced_in_neighbourhood), which is the order of the library's [E, H] export."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    grp = torch.div(torch.cumsum(g["deg"][targets], 0), max_edges, rounding_mode="floor")
    out = torch.empty(targets.numel(), g["d"], dtype=torch.float64, device=DEV)
    worst, n_edges = 0.0, 0
    try:
        for gv in torch.unique(grp).tolist():
            sel = (grp == gv).nonzero().flatten()
            ids, nts, eis, ets, tms, pos = induced_in_neighbourhood(g["ids"], g["nt"], g["ei"], g["et"], g["tm"] if g["use_rte"] else None,
                                                                    targets[sel])
            xs = g["x"][ids.flatten().to(DEV)]
            with torch.device(DEV):
                ref, att_ref = O.forward_closed_form({k: v.to(DEV) for k, v in sd.items()}, g["T"], g["R"], g["H"], xs, nts.to(DEV),
                                                     eis.to(DEV), ets.to(DEV), None if tms is None else tms.to(DEV),
                                                     use_norm=g["use_norm"], use_RTE=g["use_rte"], dtype=torch.float64, return_att=True,
                                                     dense=dense)
            out[sel] = ref[pos.to(DEV)]
            if att is not None:
                flag = torch.zeros(g["N"], dtype=torch.bool, device=DEV)
                flag[targets[sel]] = True
                eids = flag[g["ei"][1]].nonzero().flatten()
                assert eids.numel() == att_ref.size(0)
                if eids.numel():
                    worst = max(worst, (att[eids].double() - att_ref).abs().max().item())
                n_edges += int(eids.numel())
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    return out, worst, n_edges


def _forward(layer, g, flags, workspace=None):
    layer.kernel_flags = flags
    with torch.no_grad():
        out = layer(g["x"], g["nt"], g["ei"], g["et"], g["tm"] if g["use_rte"] else None,
                    n_q_rows=g["NQ"] if g["NQ"] < g["N"] else None, workspace=workspace)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c,precision", CASE_PARAMS)
def test_forward_route_case_against_fp64(c, precision):
    """One case of the list ("size line -> kernel on each side"): default flags, output of ~2000
    check rows against the fp64 closed form within PREC_TOL, attention weights of all their in-edges within 1e-5 (keep_att cases),
    rows of unknown type exactly 0, a second forward bit-identical outside the hub rows, and the default output bit-identical to
    the run that forces the expected form (all rows with HGT_FLAG_DETERMINISTIC_HUBS on both, non-hub rows without).  Cases with
    32-column heads that keep the attention weights, and the K-side cases, also run with the K-side logits kernel forced on and
    off: the default weights equal, bit for bit, the run of the kernel the route names, the two forced runs differ where the
    kernel covers the layer and are identical where it does not."""
    if HGTConv.EXTRA_KERNEL_FLAGS:
        pytest.skip("a forced-kernel pass of the suite puts one kernel on every layer: the default route under test does not run")
    t0 = time.time()
    K = _source_constants()
    N, NQ, E, d, H, T, R, dense = c["N"], c["NQ"], c["E"], c["d"], c["H"], c["T"], c["R"], c["dense"]
    route = _case_route(c, precision)
    print("\n%s %s: N=%d NQ=%d E=%d d=%d H=%d T=%d R=%d norm=%s rte=%s att=%s%s" % (
        c["id"], precision, N, NQ, E, d, H, T, R, c["use_norm"], c["use_rte"], c["keep_att"], " own workspace" if c["own_ws"] else ""))
    print("  predicate: NQ >= FUSED_MIN_NODES %s | NQ <= %d %s | N < ITEM_AGG_MAX_NODES %s | NQ < ITEM_AGG_MAX_NODES %s | scratch %d B <= 2^%d %s "
          "| R < %d %s | NQ < %d %s | dp %d" % (NQ >= K["FUSED_MIN_NODES"], K["TPW1_MAX_TARGETS"], NQ <= K["TPW1_MAX_TARGETS"],
                                               N < K["ITEM_AGG_MAX_NODES"], NQ < K["ITEM_AGG_MAX_NODES"], route["item_scratch_bytes"],
                                               K["ITEM_SCRATCH_MAX_LOG2"], route["item_scratch_bytes"] <= 1 << K["ITEM_SCRATCH_MAX_LOG2"],
                                               K["ITEM_MAX_RELATIONS"], R < K["ITEM_MAX_RELATIONS"], K["SMALL_SUB_NODES"], NQ < K["SMALL_SUB_NODES"],
                                               route["dp"]))
    print("  route: %s" % route)
    for k, v in c["expect"].items():
        assert route[k] == v, (k, route)
    g = _graph(c, seed=N % 1000 + E % 977 + d)
    sd = O.make_state_dict(d, d, T, R, H, c["use_norm"], c["use_rte"], seed=N % 13 + d, dense=dense)
    layer = _layer_from(sd, d, T, R, H, c["use_norm"], c["use_rte"], keep_att=c["keep_att"], precision=precision, dense=dense)
    GraphPlan.clear_cache()
    ws = ws_det = None
    if c["own_ws"]:           # sized without the scratch of the item-parallel form: the call falls to the sub-tile kernel
        ws = torch.empty(layer.workspace_bytes(N, E, staged=True), dtype=torch.uint8, device=DEV)
        assert ws.numel() < layer.workspace_bytes(N, E, staged=False)
        layer.kernel_flags = _lib.HGT_FLAG_DETERMINISTIC_HUBS
        ws_det = torch.empty(layer.workspace_bytes(N, E, staged=True), dtype=torch.uint8, device=DEV)
    out = _forward(layer, g, 0, ws)
    att = layer.att
    out2 = _forward(layer, g, 0, ws)
    assert out.shape == (NQ, d) and bool(torch.isfinite(out).all())
    hub_rows = g["deg"][:NQ] > K["HUB_DEG"]
    assert int(hub_rows.sum()) == 1 and bool(hub_rows[g["hub"]])
    assert torch.equal(out[~hub_rows], out2[~hub_rows]), "a second forward differs outside the hub rows"
    # check rows: pick_check_targets + the hub, the rows on both sides of the line, the last workgroup
    tg = pick_check_targets(g["nt_clean"][:NQ], g["ei"][1], n_random=1800, seed=N % 7)
    extra = [g["hub"], 0, NQ - 1] + ([c["line"] - 2, c["line"] - 1, c["line"]] if c["line"] else [])
    extra = torch.tensor([r for r in extra if 0 <= r < NQ], device=DEV)
    tg = torch.unique(torch.cat([tg, extra, torch.arange(max(0, NQ - 64), NQ, device=DEV)]))
    unknown = (g["nt"][tg] < 0) | (g["nt"][tg] >= T)
    n_last = int((tg >= NQ - 64).sum())
    assert tg.numel() >= 1000 and int(unknown.sum()) > 0 and int(g["deg"][tg].max()) > K["HUB_DEG"] and n_last >= min(64, NQ)
    if c["line"] and c["line"] - 1 < NQ:
        assert bool((tg == c["line"] - 1).any())
    if dense or c["keep_att"]:
        ref, err_att, n_att = _fp64_rows_att(sd, g, tg, dense, att if c["keep_att"] else None)
    else:
        ref, err_att, n_att = _fp64_rows(sd, g, tg), 0.0, 0
    err = (out[tg].double() - ref).abs().max().item()
    all_unknown = (g["nt"][:NQ] < 0) | (g["nt"][:NQ] >= T)
    zero_ok = bool((out[all_unknown] == 0).all())
    print("  %d check rows (%d of unknown type, %d of the last 64, max in-degree %d): max|err| vs float64 %.2e (bound %.0e)%s" % (
        tg.numel(), int(unknown.sum()), n_last, int(g["deg"][tg].max()), err, PREC_TOL[precision],
        ", attention weights of %d in-edges %.2e (bound %.0e)" % (n_att, err_att, ATT_TOL) if c["keep_att"] else ""))
    # the default route against the forced expected form
    n_diff = n_diff_det = -1
    if precision != "fp32":
        ff = _forcing_flags(route["agg"])
        forced = _forward(layer, g, ff, ws)
        det = _forward(layer, g, _lib.HGT_FLAG_DETERMINISTIC_HUBS, ws_det)
        forced_det = _forward(layer, g, ff | _lib.HGT_FLAG_DETERMINISTIC_HUBS, ws_det)
        n_diff = int((out[~hub_rows] != forced[~hub_rows]).any(dim=1).sum())
        n_diff_det = int((det != forced_det).any(dim=1).sum())
        err_det = (det[tg].double() - ref).abs().max().item()
        print("  forced %s (flags %d): %d non-hub rows differ from the default run; with deterministic hubs %d rows differ, max|err| %.2e"
              % (route["agg"], ff, n_diff, n_diff_det, err_det))
    # the logits kernel, read off the bits of the attention weights: hgt_edge_logits_kside rounds differently from the target-side
    # kernels, so on a layer it covers the two forced runs differ and the default run equals the one the route names; on a layer it
    # does not cover both flags are ignored.  (The forcing flags of the aggregation above name no logits kernel.)
    n_att_diff, att_runs = -1, None
    if c["keep_att"] and (route["dkp"] == K["KSIDE_DK"] or c.get("logits_bits")):
        det_fl = _lib.HGT_FLAG_DETERMINISTIC_HUBS
        att_runs = []
        for fl in (det_fl, det_fl | _lib.HGT_FLAG_KSIDE_LOGITS, det_fl | _lib.HGT_FLAG_NO_KSIDE_LOGITS):
            _forward(layer, g, fl, ws_det)
            att_runs.append(layer.att.view(torch.int32))
        n_att_diff = int((att_runs[1] != att_runs[2]).sum())
        print("  logits %s (covered by the K-side kernel: %s): %d of %d attention weights differ between the runs forced to it and off it"
              % (route["logits"], route["kside_covered"], n_att_diff, att_runs[1].numel()))
    print("  %.3f s" % (time.time() - t0))
    GraphPlan.clear_cache()
    assert err < PREC_TOL[precision]
    assert zero_ok, "rows of unknown type must be exactly 0"
    if c["keep_att"]:
        assert att is not None and att.shape == (E, H) and n_att > 0
        assert err_att < ATT_TOL
    if precision != "fp32":
        assert n_diff == 0, "the default route is not the expected form %s: %d rows differ from the forced run" % (route["agg"], n_diff)
        assert n_diff_det == 0
        assert err_det < PREC_TOL[precision]
    if att_runs is not None:
        assert route["logits"] in ("kside", "valu")
        want = att_runs[1] if route["logits"] == "kside" else att_runs[2]
        assert torch.equal(att_runs[0], want), "the default route's logits kernel is not %s" % route["logits"]
        not_hub = ~hub_rows[g["ei"][1]]         # (without deterministic hubs: every edge into a non-hub row)
        assert torch.equal(att.view(torch.int32)[not_hub], want[not_hub]), "the default run's logits kernel is not %s" % route["logits"]
        if route["kside_covered"]:
            assert n_att_diff > 0, "the forced runs are bit-identical: the comparison says nothing about the logits kernel"
        else:
            assert n_att_diff == 0 and torch.equal(att_runs[0], att_runs[1])
