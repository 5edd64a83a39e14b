"""GPU tests of the backward primitives one by one (include/hgt_hip.h, the block above hgt_edge_spmm): each is called through
the C ABI on dense random inputs (non-zero everywhere, so that a dropped wavefront, item or flush changes the result) and
compared with its float64 restatement in oracle/backward_primitives.py.  Accumulating outputs are pre-filled (the += contract),
strided outputs carry sentinels in their padding, and every case asserts the size branch of the kernel it is meant to reach by
recomputing the host-side predicate (a retuned threshold then fails here instead of silently dropping coverage)."""
import ctypes as C

import pytest
import torch

from oracle import backward_primitives as BP
from pyhgt_amd import GraphPlan, _lib
from pyhgt_amd.autograd import spmm_takes_items

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HGT_ERR_UNSUPPORTED = -2


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _close(name, got, ref, rtol, entry_rtol=None):
    """max |got - ref| <= rtol * max |ref|, and per entry |got - ref| <= entry_rtol * (|ref| + rms(ref))."""
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite entries" % name
    diff = (got - ref).abs()
    scale = max(ref.abs().max().item(), 1e-30)
    err = diff.max().item() / scale
    assert err <= rtol, "%s: max |kernel - fp64| = %.3e of the largest entry (%.3e)" % (name, err, scale)
    if entry_rtol is not None:
        rms = ref.pow(2).mean().sqrt().item()
        excess = (diff - entry_rtol * (ref.abs() + rms)).max().item()
        assert excess <= 0.0, "%s: an entry misses %.0e * (|ref| + rms) by %.3e" % (name, entry_rtol, excess)
    return err


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g):
    """Dense random values bounded away from zero (|v| >= 0.05): a missing term can never hide behind a zero input."""
    v = torch.randn(shape, generator=g, device=DEV)
    return torch.where(v.abs() < 0.05, torch.where(v < 0, -0.05, 0.05), v)


# ------------------------------------------------------------------------------------------------------------------------------
# hgt_node_update_bwd / hgt_node_update_bwd_ex
# ------------------------------------------------------------------------------------------------------------------------------
def nub_rows_per_wave(n_rows):
    # mirrors nub_plan of pyhgt_amd/csrc/hgt_bwd_update.hip
    return 32 if n_rows >= 65536 else (8 if n_rows >= 16384 else 2)


NUB_FORMS = ["gated_norm", "gated_plain", "residual_norm", "residual_shared_norm"]
NUB_TYPES = ["shuffled", "runs7", "runs33"]
NUB_DIMS = [64, 256, 400, 512]             # 400: the last 64-column group is partial; 512 = NUB_MAXC * 64
# rows -> the rows-per-wavefront branch each is meant to reach (both sides of both thresholds)
NUB_ROWS = [(3001, 2), (16383, 2), (16384, 8), (40000, 8), (65535, 8), (65536, 32), (70001, 32)]
NUB_CASES = []
for _i, (_n, _rpw) in enumerate(NUB_ROWS):
    for _j, _form in enumerate(NUB_FORMS):
        NUB_CASES.append((_n, _rpw, _form, NUB_DIMS[(_i + _j) % 4], NUB_TYPES[(_i + 2 * _j) % 3], (_i + _j) % 2 == 1))


def test_node_update_cases_cover_every_rows_per_wave_branch():
    assert {nub_rows_per_wave(n) for n, *_ in NUB_CASES} == {2, 8, 32}
    for rpw in (2, 8, 32):      # every branch meets every update form, with and without a dropout mask
        assert {c[2] for c in NUB_CASES if c[1] == rpw} == set(NUB_FORMS)
        assert {c[5] for c in NUB_CASES if c[1] == rpw} == {False, True}


def _node_types(n, T, pattern, g):
    if pattern == "shuffled":
        nt = torch.randint(0, T, (n,), generator=g, device=DEV)
    else:
        run = 7 if pattern == "runs7" else 33          # runs crossing the 2 / 8 / 32-row wavefront boundaries
        nt = (torch.arange(n, device=DEV) // run) % T
    # unknown types mixed in: -1 and T + 1 (rows no typed layer claims: zero output, zero gradient)
    nt[torch.randint(0, n, (max(n // 19, 3),), generator=g, device=DEV)] = -1
    nt[torch.randint(0, n, (max(n // 23, 3),), generator=g, device=DEV)] = T + 1
    return nt.to(torch.int64)


@pytest.mark.parametrize("n,rpw,form,d,types,masked", NUB_CASES,
                         ids=["%d-%s-d%d-%s%s" % (c[0], c[2], c[3], c[4], "-mask" if c[5] else "") for c in NUB_CASES])
def test_node_update_bwd_matches_fp64(n, rpw, form, d, types, masked):
    assert nub_rows_per_wave(n) == rpw, "the rows-per-wavefront thresholds moved: re-aim this case"
    lib = _lib.load()
    T = 3
    g = _gen(n + d)
    gated = form.startswith("gated")
    use_norm = form != "gated_plain"
    shared = form == "residual_shared_norm"
    nt = _node_types(n, T, types, g)
    ldx, ld_dx = d + 12, d + 20
    trans = _randn((n, d), g)
    xbuf = _randn((n, ldx), g)                                  # x[:, :d] is the skip input; the rest of the row is never read
    gout = _randn((n, d), g)
    skip = torch.randn(T, generator=g, device=DEV) if gated else None
    ln_w = (1.0 + 0.2 * torch.randn(T, d, generator=g, device=DEV)) if use_norm else None
    mask = (torch.bernoulli(torch.full((n, d), 0.8, device=DEV), generator=g) / 0.8) if masked else None
    if mask is not None:
        trans = trans * mask                                   # the saved a_linear output is the dropped one (autograd.py)
    # outputs: d_trans / dx overwritten (sentinels everywhere first, also in dx's padding), the rest accumulate (+=)
    d_trans = torch.full((n, d), 7.0, device=DEV)
    dx = torch.full((n, ld_dx), -9.0, device=DEV)
    d_alpha0 = torch.randn(T, generator=g, device=DEV)
    d_lnw0 = torch.randn(T, d, generator=g, device=DEV)
    d_lnb0 = torch.randn(T, d, generator=g, device=DEV)
    d_alpha, d_lnw, d_lnb = d_alpha0.clone(), d_lnw0.clone(), d_lnb0.clone()
    args_tail = (_p(mask), n, d, T, _p(d_trans), _p(dx), ld_dx, _p(d_alpha) if gated else 0, _p(d_lnw) if use_norm else 0,
                 _p(d_lnb) if use_norm else 0, _st())
    if form.startswith("gated") and not shared:
        rc = lib.hgt_node_update_bwd(_p(gout), _p(trans), _p(xbuf), ldx, _p(nt), _p(skip), _p(ln_w), int(use_norm), *args_tail)
    else:
        rc = lib.hgt_node_update_bwd_ex(_p(gout), _p(trans), _p(xbuf), ldx, _p(nt), _p(skip), _p(ln_w), int(use_norm), int(shared),
                                        *args_tail)
    assert rc == 0
    torch.cuda.synchronize()
    ref = BP.node_update_bwd(gout, trans, xbuf, nt, T, skip=skip, ln_w=ln_w, use_norm=use_norm, shared_norm=shared, drop_mask=mask)
    unknown = (nt < 0) | (nt >= T)
    assert bool((d_trans[unknown] == 0).all()) and bool((dx[unknown, :d] == 0).all()), "rows of unknown type must be exact zeros"
    assert bool((dx[:, d:] == -9.0).all()), "dx written beyond d columns"
    _close("d_trans", d_trans, ref["d_trans"], 1e-5, 1e-4)
    _close("dx", dx[:, :d], ref["dx"], 1e-5, 1e-4)
    if gated:
        _close("d_alpha", d_alpha.double() - d_alpha0.double(), ref["d_alpha"], 1e-4, 1e-4)
    if use_norm:
        rows = 1 if shared else T
        _close("d_ln_w", d_lnw[:rows].double() - d_lnw0[:rows].double(), ref["d_ln_w"], 1e-4, 1e-4)
        _close("d_ln_b", d_lnb[:rows].double() - d_lnb0[:rows].double(), ref["d_ln_b"], 1e-4, 1e-4)
        if shared:
            assert torch.equal(d_lnw[1:], d_lnw0[1:]) and torch.equal(d_lnb[1:], d_lnb0[1:]), "shared norm wrote past row 0"


# ------------------------------------------------------------------------------------------------------------------------------
# graph-level fixtures
# ------------------------------------------------------------------------------------------------------------------------------
def _layout(d, H):
    lay = _lib.HgtLayout()
    assert _lib.load().hgt_layout_for(d, H, C.byref(lay)) == 0
    return lay


def _max_items(N, E, T, R):
    sz = _lib.HgtPlanSizes()
    assert _lib.load().hgt_plan_sizes_for(N, E, T, R, C.byref(sz)) == 0
    return int(sz.max_items)


def _graph(N, E, T, R, seed, rte=True, hubs=False, unknown=True, unclaimed=True, empty_rel=None, sorted_types=False):
    """Device graph with unknown node types, unclaimed edges (relation R), optionally a relation with no edges, a target with
    > 1024 in-edges and a source with > 1024 out-edges (a hub of the transposed plan)."""
    g = _gen(seed)
    nt = torch.randint(0, T, (N,), generator=g, device=DEV)
    if sorted_types:
        nt = nt.sort().values
    src = torch.randint(0, N, (E,), generator=g, device=DEV)
    dst = torch.randint(0, N, (E,), generator=g, device=DEV)
    et = torch.randint(0, R, (E,), generator=g, device=DEV)
    tm = torch.randint(0, 240, (E,), generator=g, device=DEV)
    if unknown:
        nt[torch.randint(0, N, (N // 29 + 1,), generator=g, device=DEV)] = -1
        nt[torch.randint(0, N, (N // 31 + 1,), generator=g, device=DEV)] = T + 1
    if unclaimed:
        et[::17] = R
    if empty_rel is not None:
        et[et == empty_rel] = (empty_rel + 1) % R
    if hubs:
        dst[:1500] = 17
        src[2000:3600] = 23
    ei = torch.stack([src, dst], dim=1).t()          # the (1,2)-strided view of the reference's data path
    return nt, ei, et, (tm if rte else None)


def _frags(f_p, R, H, dkp):
    lib = _lib.load()
    nb = C.c_uint64()
    assert lib.hgt_relation_frag_bytes(R, H, dkp, C.byref(nb)) == 0
    assert nb.value > 0
    frag = torch.empty(int(nb.value), dtype=torch.uint8, device=DEV)
    assert lib.hgt_relation_frag_pack(f_p.data_ptr(), R, H, dkp, frag.data_ptr(), _st()) == 0
    return frag


def _to_sorted(plan, by_id, T, R):
    out = torch.empty_like(by_id)
    assert _lib.load().hgt_edge_gather_sorted(plan.ptr, plan.N, plan.E, T, R, by_id.size(1), by_id.data_ptr(), out.data_ptr(), _st()) == 0
    return out


def _to_edge_ids(plan, sorted_vals, T, R):
    out = torch.empty_like(sorted_vals)
    H = sorted_vals.size(1)
    assert _lib.load().hgt_att_export(plan.ptr, plan.N, plan.E, T, R, H, sorted_vals.data_ptr(), out.data_ptr(), H, _st()) == 0
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# hgt_relation_outer
# ------------------------------------------------------------------------------------------------------------------------------
def outer_items_per_wave_factor(max_items):
    # mirrors outer_items_per_wave of pyhgt_amd/csrc/hgt_bwd_outer.hip: 2 (R + 1) items per wavefront below 16 384 items, else 16 (R + 1)
    return 2 if max_items < 16384 else 16


def outer_form(lay):
    # mirrors outer_lane_split of hgt_bwd_outer.hip: the split of a head over lanes
    lph = 64 // lay.heads
    vec, l2 = lay.dk_pad // lph, lph
    while vec * lay.dk_pad > 128 and vec > 1 and l2 * 2 <= 64:
        vec, l2 = vec // 2, l2 * 2
    if not (vec * l2 * vec <= 128 and vec * l2 >= 4):
        return "unsupported"
    return "mfma" if (vec * l2 == 32 and vec <= 4) else "valu"


OUTER_CASES = [
    # name, d, H, T, R, N, E, rte, expected form, expected items-per-wavefront factor
    ("valu16_r1_small", 64, 4, 3, 1, 3000, 24000, True, "valu", 2),
    ("valu16_r8_small_plain", 64, 4, 3, 8, 5000, 40000, False, "valu", 2),
    ("valu16_r33_large", 64, 4, 3, 33, 70000, 500000, True, "valu", 16),
    ("valu16_r33_large_plain", 64, 4, 3, 33, 70000, 500000, False, "valu", 16),
    ("valu64_r8_small", 256, 4, 3, 8, 4000, 30000, True, "valu", 2),
    ("valu64_r33_large", 256, 4, 3, 33, 66000, 500000, True, "valu", 16),
    ("valu64_r33_large_plain", 256, 4, 3, 33, 66000, 500000, False, "valu", 16),
    ("mfma_d256h8_small", 256, 8, 4, 8, 4000, 40000, True, "mfma", 2),
    ("mfma_d256h8_large_rte", 256, 8, 4, 33, 66000, 500000, True, "mfma", 16),
    ("mfma_d256h8_large_plain", 256, 8, 4, 33, 66000, 500000, False, "mfma", 16),
    ("mfma_d96h3_small_plain", 96, 3, 2, 8, 3000, 24000, False, "mfma", 2),
    ("mfma_d96h3_large_rte", 96, 3, 2, 33, 70000, 500000, True, "mfma", 16),
    ("mfma_d96h3_large_plain", 96, 3, 2, 33, 70000, 500000, False, "mfma", 16),
]


def test_relation_outer_cases_cover_both_regimes_of_both_forms():
    seen = {(c[8], c[9], c[7]) for c in OUTER_CASES}                      # (form, items-per-wavefront factor, RTE)
    assert {(f, 16, r) for f in ("valu", "mfma") for r in (True, False)} <= seen
    assert {(f, 2) for f in ("valu", "mfma")} <= {(f, i) for f, i, _ in seen}
    assert {c[4] for c in OUTER_CASES} >= {1, 8, 33}


@pytest.mark.parametrize("case", OUTER_CASES, ids=[c[0] for c in OUTER_CASES])
def test_relation_outer_matches_fp64(case):
    name, d, H, T, R, N, E, rte, form, ipw = case
    lib = _lib.load()
    lay = _layout(d, H)
    assert outer_form(lay) == form, "the head split of hgt_relation_outer moved: re-aim %s" % name
    assert outer_items_per_wave_factor(_max_items(N, E, T, R)) == ipw, "the items-per-wavefront threshold moved: re-aim %s" % name
    Hl, dkp, dp = lay.heads, lay.dk_pad, lay.d_pad
    nt, ei, et, tm = _graph(N, E, T, R, seed=N + R + d, rte=rte, empty_rel=min(1, R - 1) if R > 1 else None)
    plan = GraphPlan(nt, ei, et, tm, T, R)
    g = _gen(d + H)
    w_id = _randn((E, Hl), g)
    a = _randn((N, dp), g)
    b = _randn((N, dp), g)
    rte_a = _randn((T * 240, dp), g) if rte else None
    out0 = torch.randn(R, Hl, dkp, dkp, generator=g, device=DEV)
    out = out0.clone()
    w = _to_sorted(plan, w_id, T, R)                     # weights by edge id -> plan order
    assert lib.hgt_relation_outer(plan.ptr, N, E, T, R, Hl, dkp, w.data_ptr(), a.data_ptr(), _p(rte_a), b.data_ptr(), out.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    src, dst, rel, rrow = BP.plan_edges(nt, ei, et, tm, T, R)
    ref = BP.relation_outer(src, dst, rel, rrow, w_id, a, rte_a, b, R, Hl, dkp)
    got = out.double() - out0.double()
    if R > 1:
        assert bool((rel == 1).sum() == 0) and torch.equal(out[1], out0[1]), "a relation without edges must stay untouched"
    _close("relation_outer", got, ref, 2e-5, 1e-4)


def test_relation_outer_rejects_128_column_heads():
    lib = _lib.load()
    T, R, N, E, d, H = 2, 3, 500, 3000, 512, 4
    lay = _layout(d, H)
    assert lay.dk_pad == 128 and outer_form(lay) == "unsupported"
    nt, ei, et, _ = _graph(N, E, T, R, seed=3, rte=False)
    plan = GraphPlan(nt, ei, et, None, T, R)
    w = torch.ones(E, lay.heads, device=DEV)
    a = torch.ones(N, lay.d_pad, device=DEV)
    out = torch.zeros(R, lay.heads, 128, 128, device=DEV)
    assert lib.hgt_relation_outer(plan.ptr, N, E, T, R, lay.heads, 128, w.data_ptr(), a.data_ptr(), 0, a.data_ptr(), out.data_ptr(),
                                  _st()) == HGT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# hgt_edge_spmm / hgt_edge_spmm_items on a plan and on its transposed plan
# ------------------------------------------------------------------------------------------------------------------------------
SPMM_CASES = [
    # name, d, H, T, R, N, E, rte, n_q_rows (None = N)
    ("d64h4_r4_rte", 64, 4, 3, 4, 5000, 60000, True, None),
    ("d256h8_r9_plain", 256, 8, 4, 9, 6000, 60000, False, None),
    ("d96h3_r5_rte_nq", 96, 3, 2, 5, 6000, 50000, True, 4100),
    ("d400h8_r33_rte_big", 400, 8, 3, 33, 70000, 400000, True, None),
    ("d256h8_r8_plain_big", 256, 8, 4, 8, 66000, 400000, False, None),
]


def test_spmm_cases_straddle_the_gather_pass_threshold():
    # autograd's choice between the two kernels (autograd.spmm_takes_items): hgt_edge_spmm_items below 65 536 nodes; the cases write
    # the second d_pad-wide block of rows of 2 d_pad columns
    takes = {spmm_takes_items(c[5], c[6], c[4], 2 * _layout(c[1], c[2]).d_pad, _layout(c[1], c[2]).d_pad) for c in SPMM_CASES}
    assert takes == {c[5] < 65536 for c in SPMM_CASES} == {True, False}
    assert {c[7] for c in SPMM_CASES} == {True, False}


@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "transposed"])
@pytest.mark.parametrize("case", SPMM_CASES, ids=[c[0] for c in SPMM_CASES])
def test_edge_spmm_kernels_match_fp64(case, transposed):
    name, d, H, T, R, N, E, rte, nq = case
    lib = _lib.load()
    lay = _layout(d, H)
    Hl, dkp, dp = lay.heads, lay.dk_pad, lay.d_pad
    nt, ei, et, tm = _graph(N, E, T, R, seed=E + d, rte=rte, hubs=True)
    if nq is not None:
        ei = ei.clone()
        ei[1 if not transposed else 0] %= nq                      # every target of the plan below n_q_rows
    NQ = N if nq is None else nq
    plan = GraphPlan(nt, ei, et, tm, T, R, n_q_rows=nq, reverse=transposed)
    src, dst, rel, rrow = BP.plan_edges(nt, ei, et, tm, T, R, reverse=transposed)
    deg_in = torch.bincount(dst, minlength=N)
    assert deg_in.max().item() > 1024, "no hub target in this plan"
    g = _gen(N + R)
    w_id = _randn((E, Hl), g)
    rows = _randn((N, dp), g)
    rte_rows = _randn((T * 240, dp), g) if rte else None
    f_p = (torch.randn(R, Hl, dkp, dkp, generator=g, device=DEV) / dkp ** 0.5)
    frag = _frags(f_p, R, Hl, dkp)
    w = _to_sorted(plan, w_id, T, R)
    ref = BP.edge_spmm(src, dst, rel, rrow, w_id, rows, rte_rows, f_p, NQ, R, Hl, dkp)
    nb = C.c_uint64()
    assert lib.hgt_hub_workspace_bytes(E, Hl, dkp, C.byref(nb)) == 0
    hub = torch.empty(max(int(nb.value), 256), dtype=torch.uint8, device=DEV)
    assert lib.hgt_edge_aggregate_items_bytes(E, Hl, dkp, C.byref(nb)) == 0
    scratch = torch.empty(max(int(nb.value), 16), dtype=torch.uint8, device=DEV)
    for kernel in ("spmm", "spmm_items"):
        out = torch.full((NQ, 2 * dp), 5.0, device=DEV)            # written into the second column block: ld_out = 2 dp
        optr = out.data_ptr() + 4 * dp
        if kernel == "spmm":
            rc = lib.hgt_edge_spmm(plan.ptr, N, E, T, R, Hl, dkp, w.data_ptr(), rows.data_ptr(), _p(rte_rows), f_p.data_ptr(),
                                   frag.data_ptr(), optr, 2 * dp, NQ, hub.data_ptr(), _st())
        else:
            rc = lib.hgt_edge_spmm_items(plan.ptr, N, E, T, R, Hl, dkp, w.data_ptr(), rows.data_ptr(), _p(rte_rows), frag.data_ptr(),
                                         optr, 2 * dp, NQ, scratch.data_ptr(), scratch.numel(), _st())
        assert rc == 0, (kernel, rc)
        torch.cuda.synchronize()
        assert bool((out[:, :dp] == 5.0).all()), "%s wrote outside its column block" % kernel
        # split-bf16 x3 products (relative error of a product ~3 * 2^-18): 2e-5 of the largest entry, like the forward
        _close("%s/%s" % (kernel, "transposed" if transposed else "plan"), out[:, dp:], ref, 2e-5)


# ------------------------------------------------------------------------------------------------------------------------------
# hgt_edge_softmax_bwd, hgt_head_dot, hgt_gelu_bwd
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", [(64, 4), (96, 3), (256, 8)])
def test_softmax_bwd_and_head_dot_match_fp64(d, H):
    lib = _lib.load()
    T, R, N, E = 3, 5, 20000, 120000
    lay = _layout(d, H)
    Hl, dkp, dp = lay.heads, lay.dk_pad, lay.d_pad
    nt, ei, et, tm = _graph(N, E, T, R, seed=d, rte=False, hubs=True)
    plan = GraphPlan(nt, ei, et, None, T, R)
    src, dst, rel, _ = BP.plan_edges(nt, ei, et, None, T, R)
    g = _gen(H)
    # rows with the layout's padding (extra heads / columns beyond d_k) at zero, like the training path's dagg / agg
    live = torch.zeros(Hl, dkp, dtype=torch.bool, device=DEV)
    live[:H, :lay.d_k] = True
    live = live.flatten()
    a = _randn((N, dp), g) * live
    b = _randn((N, dp), g) * live
    rho = torch.full((N, Hl), 3.0, device=DEV)
    assert lib.hgt_head_dot(a.data_ptr(), b.data_ptr(), N, Hl, dkp, rho.data_ptr(), _st()) == 0
    att_id = torch.rand(E, Hl, generator=g, device=DEV) + 0.01
    att_id[:, H:] = 0.0                                           # extra layout heads carry no attention
    datt_id = _randn((E, Hl), g)
    ds = torch.full((E, Hl), 11.0, device=DEV)
    att_s, datt_s = _to_sorted(plan, att_id, T, R), _to_sorted(plan, datt_id, T, R)
    assert lib.hgt_edge_softmax_bwd(plan.ptr, N, E, T, R, Hl, att_s.data_ptr(), datt_s.data_ptr(), rho.data_ptr(), Hl, ds.data_ptr(),
                                    _st()) == 0
    ds_id = _to_edge_ids(plan, ds, T, R)
    torch.cuda.synchronize()
    rho_ref = BP.head_dot(a, b, Hl, dkp)
    _close("head_dot", rho, rho_ref, 1e-5, 1e-4)
    assert bool((rho[:, H:] == 0).all()), "padded heads must stay zero"
    _close("edge_softmax_bwd", ds_id, BP.edge_softmax_bwd(att_id, datt_id, rho.double(), dst), 1e-6, 1e-5)
    assert bool((ds_id[:, H:] == 0).all())
    assert torch.bincount(dst, minlength=N).max().item() > 1024


def test_gelu_bwd_matches_fp64():
    lib = _lib.load()
    g = _gen(1)
    x = torch.cat([torch.linspace(-10.0, 10.0, 40001, device=DEV), torch.linspace(-1e-3, 1e-3, 2001, device=DEV),
                   torch.tensor([0.0, -0.0, 1e-7, -1e-7, 1e-30, 6.0, -6.0, 9.99, -9.99], device=DEV),
                   10.0 * (2.0 * torch.rand(100000, generator=g, device=DEV) - 1.0)])
    x = x[: x.numel() // 4 * 4].contiguous()
    dg = _randn((x.numel(),), g)
    out = torch.full_like(x, 13.0)
    assert lib.hgt_gelu_bwd(dg.data_ptr(), x.data_ptr(), out.data_ptr(), x.numel(), _st()) == 0
    torch.cuda.synchronize()
    ref = BP.gelu_bwd(dg, x)
    diff = (out.double() - ref).abs()
    excess = (diff - (1e-6 * dg.abs().double() + 1e-5 * ref.abs())).max().item()
    assert excess <= 0.0, "gelu_bwd misses 1e-6 |dg| + 1e-5 |ref| by %.3e" % excess


# ------------------------------------------------------------------------------------------------------------------------------
# hgt_att_export o hgt_edge_gather_sorted: a bit-exact round trip, and a permutation
# ------------------------------------------------------------------------------------------------------------------------------
def item_edges(E):
    # mirrors hgt_item_edges, pyhgt_amd/csrc/hgt_common.h:71 (HGT_CH = 512, HGT_MIN_ITEM = 16)
    ch = 512
    while ch > 16 and E // ch < 4096:
        ch >>= 1
    return ch


@pytest.mark.parametrize("E,ch", [(60000, 16), (300000, 64), (2200000, 512)])
def test_att_export_inverts_edge_gather_sorted(E, ch):
    assert item_edges(E) == ch, "the work-item length thresholds moved: re-aim this case"
    T, R, N, H = 3, 6, max(E // 10, 1000), 4
    nt, ei, et, tm = _graph(N, E, T, R, seed=E, rte=True, hubs=True)
    plan = GraphPlan(nt, ei, et, tm, T, R)
    g = _gen(E)
    by_id = torch.randn(E, H, generator=g, device=DEV)
    srt = _to_sorted(plan, by_id, T, R)
    back = _to_edge_ids(plan, srt, T, R)
    ids = torch.arange(E, device=DEV, dtype=torch.float32).unsqueeze(1).repeat(1, H)   # exact in fp32 below 2^24
    perm = _to_sorted(plan, ids, T, R)
    torch.cuda.synchronize()
    assert torch.equal(back, by_id)
    p = perm[:, 0].to(torch.int64)
    assert torch.equal(perm, p.to(torch.float32).unsqueeze(1).repeat(1, H))
    assert torch.equal(torch.sort(p).values, torch.arange(E, device=DEV)), "gather_sorted is not a permutation of the edges"
    # plan order groups by (target tile, relation): the targets of consecutive sorted edges never go back to an earlier tile
    src, dst, rel, _ = BP.plan_edges(nt, ei, et, tm, T, R)
    tiles = dst[p] // 256
    assert bool((tiles[1:] >= tiles[:-1]).all())
