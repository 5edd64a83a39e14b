"""GPU tests of the code above and beside HGTConv at full-graph sizes, against float64 (run with -m gpu on an MI355X):
the slab GEMM variants only full graphs reach, hgt_tanh_inplace, the GNN stack on both sides of the 65 536-node line, the plan's
row lists at the one-workgroup kernel's limit, and the Classifier / Matcher heads at real shapes, forward and backward.
Every case recomputes the size predicate of the branch it targets from the code's constants, asserts it and prints it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import hgt_oracle as O
from pyhgt_amd import GraphPlan, _lib
from pyhgt_amd.synth import pick_check_targets, synthetic_typed_graph
from test_hgt_gpu import DEV, PREC_TOL, _fp64_rows, _plan_arrays, _to_dev

pytestmark = pytest.mark.gpu

# constants of the code under test (pyhgt_amd/csrc): a retuned threshold makes the predicate assertions below fail loudly
BM, BNP, KP = 64, 256, 256                  # hgt_split_common.h: rows per workgroup, columns per pass, K panel
TILE_MAX_ROWS = 16384                       # hgt_gemm_tile.hip HGT_TILE_MAX_ROWS
XS_K = (64, 128, 256, 512)                  # hgt_gemm_xs.hip: the K the x-stationary kernel takes
ITEM_AGG_MAX_NODES = 65536                  # hgt_api.hip HGT_ITEM_AGG_MAX_NODES (NQ < this: item-parallel aggregation)
SMALL_ROWS_N, SMALL_ROWS_T = 65536, 30      # hgt_plan.hip: one-workgroup row lists for N <= 65536 and T <= 30
ADAPTER_EPILOGUE_MAX_N = 65536              # model.py: GNN.forward asks for the tanh epilogue below this many nodes
HGT_ERR_INVALID_ARG = -1
SENTINEL = -7777.0


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count        # pc_grid() of hgt_gemm_bf16x3.hip


def _split_dispatch(n_rows, T, k, n_out, vec_ok, tanh=False):
    """The kernel typed_linear_split_impl (hgt_gemm_bf16x3.hip) picks for a plain-prologue call, restated in Python."""
    row_tiles = (n_rows + BM - 1) // BM + T
    n_pass = (n_out + BNP - 1) // BNP
    pass_split = n_pass if (n_pass > 1 and row_tiles * 2 <= _n_cu()) else 1
    d = dict(row_tiles=row_tiles, pass_split=pass_split, vec_ok=vec_ok)
    if n_rows <= TILE_MAX_ROWS:
        d["kernel"] = "tile"
    elif tanh and k <= KP:
        d["kernel"] = "unsupported"
    elif not tanh and vec_ok and k in XS_K and 64 < n_out <= 3072 and n_rows >= (65536 if k == 512 else 262144):
        d["kernel"] = "xs"
    elif k <= KP:
        grid = min(row_tiles * pass_split, _n_cu())
        d.update(kernel="persistent", rounds=(row_tiles * pass_split + grid - 1) // grid)
    else:
        d.update(kernel="slab", nstg=4 if row_tiles * pass_split <= 2 * _n_cu() else 2)
    return d


def _split_weights(W, f16):
    lib = _lib.load()
    G, n_out, k = W.shape
    nb = C.c_uint64()
    assert lib.hgt_split_weights_bytes(G, k, n_out, C.byref(nb)) == 0
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=DEV)
    split = lib.hgt_split_weights_f16 if f16 else lib.hgt_split_weights
    assert split(W.data_ptr(), n_out * k, G, k, n_out, ws.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return ws


def _gemm_tol(f16, k):
    return (4e-6 if f16 else 1e-4) * math.ceil(k / 256)      # test_xs_gemm_against_fp64_at_its_dispatch_sizes, per 256 of K


# ------------------------------------------------------------------ 1. slab GEMM variants that only full graphs reach
GEMM_CASES = [
    (70_001, 400, 1200, 4, "plain", dict(kernel="slab", nstg=2, pass_split=1)),       # OAG Q|K|V, 3 output blocks
    (65_535, 1169, 400, 5, "tanh", dict(kernel="slab", nstg=2, pass_split=1)),        # OAG adapter with the tanh epilogue
    (90_001, 800, 400, 1, "gelu", dict(kernel="slab", nstg=2, pass_split=1)),         # DenseHGTConv out_linear at d = 400
    (200_003, 768, 2304, 3, "plain", dict(kernel="slab", nstg=2, pass_split=1)),      # d = 768 projections
    (300_007, 129, 512, 4, "plain", dict(kernel="persistent", vec_ok=0)),             # ogbn-mag adapter
    (300_007, 256, 768, 4, "offset", dict(kernel="persistent", vec_ok=0)),            # K = 256 rows not 16-byte aligned
]


@pytest.mark.parametrize("precision", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("N,k,n_out,T,mode,expect", GEMM_CASES, ids=["%d-%d-%d-%s" % (c[0], c[1], c[2], c[4]) for c in GEMM_CASES])
def test_slab_gemm_variants_of_full_graphs_against_fp64(N, k, n_out, T, mode, expect, precision):
    """hgt_typed_linear_bf16x3 / _f16x3 where only full graphs take them: the non-deep (NSTG = 2) K > 256 slab kernel, with the
    gelu prologue and the tanh epilogue, and the persistent kernel without 16-byte rows at many rounds per workgroup.  Ragged,
    permuted row lists with an empty group that leave 1/64 of the rows out: those rows keep their fill value.  The tanh epilogue
    must equal the plain call followed by hgt_tanh_inplace bit for bit (the two forms of GNN.forward's adapter)."""
    lib = _lib.load()
    f16 = precision == "f16x3"
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(N % 97 + k)
    gd = torch.Generator(device=DEV).manual_seed(N + k)
    if mode == "offset":
        xbuf = torch.randn(N * k + 1, generator=gd, device=DEV)
        x = xbuf[1:].view(N, k)
        assert x.data_ptr() % 16 != 0
    else:
        x = torch.randn(N, k, generator=gd, device=DEV)
    W = (torch.randn(T, n_out, k, generator=g) / k ** 0.5).to(DEV)
    b = torch.randn(T, n_out, generator=g).to(DEV)
    n_list = N - N // 64
    rows = torch.randperm(N, generator=g)[:n_list].to(torch.int32).to(DEV)
    cuts = sorted(torch.randint(0, n_list, (T - 1,), generator=g).tolist())
    if T >= 4:                                   # an empty group and a 37-row one
        cuts[1] = cuts[0]
        cuts[2] = min(n_list, cuts[1] + 37)
        cuts = sorted(cuts)
    off = torch.tensor([0] + cuts + [n_list], dtype=torch.int32, device=DEV)
    vec_ok = int(k % 4 == 0 and x.data_ptr() % 16 == 0)
    d = _split_dispatch(n_list, T, k, n_out, vec_ok, tanh=(mode == "tanh"))
    print("\nN=%d k=%d n_out=%d T=%d %s: dispatch %s" % (N, k, n_out, T, mode, d))
    for key, v in expect.items():
        assert d[key] == v, (key, d)
    if d["kernel"] == "persistent":
        assert d["rounds"] >= 8
    ws = _split_weights(W, f16)
    nblk = 3 if (n_out % 3 == 0 and (n_out // 3) % 4 == 0) else 1
    bc = n_out // nblk
    prologue = {"gelu": 1, "tanh": _lib.HGT_LINEAR_TANH}.get(mode, 0)
    linear = lib.hgt_typed_linear_f16x3 if f16 else lib.hgt_typed_linear_bf16x3

    def run(pro):
        outs = [torch.full((N, bc), SENTINEL, device=DEV) for _ in range(nblk)]
        optr = [o.data_ptr() for o in outs] + [None, None]
        rc = linear(x.data_ptr(), k, rows.data_ptr(), off.data_ptr(), T, n_list, k, n_out, ws.data_ptr(), b.data_ptr(), n_out,
                    optr[0], optr[1], optr[2], bc, 0, pro, st)
        assert rc == 0, rc
        return torch.cat(outs, 1)

    got = run(prologue)
    torch.cuda.synchronize()
    listed = torch.zeros(N, dtype=torch.bool, device=DEV)
    listed[rows.long()] = True
    assert bool((got[~listed] == SENTINEL).all()), "a row outside the list was written"
    xin = torch.nn.functional.gelu(x.double()) if mode == "gelu" else x
    offl = off.tolist()
    worst = 0.0
    for t in range(T):
        r = rows[offl[t]:offl[t + 1]].long()
        for lo in range(0, r.numel(), 65536):
            rr = r[lo:lo + 65536]
            ref = xin[rr].double() @ W[t].double().T + b[t].double()
            if mode == "tanh":
                ref = torch.tanh(ref)
            worst = max(worst, float((got[rr].double() - ref).abs().max()))
    tol = _gemm_tol(f16, k)
    print("%s: max|err| vs float64 %.2e (bound %.1e)" % (precision, worst, tol))
    assert worst < tol
    if mode == "tanh":
        plain = run(0)
        assert lib.hgt_tanh_inplace(plain.data_ptr(), plain.numel(), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(got[listed], plain[listed]), "tanh epilogue and plain call + hgt_tanh_inplace differ"


# ------------------------------------------------------------------ 2. hgt_tanh_inplace against torch.tanh in float64
TANH_REL_TOL = 4e-7         # relative error on every normal input: measured 2.05e-7 on an MI355X (the exp2 / rcp form at |x| ~ 0.37)
TANH_ABS_TOL = 2e-7
FLT_MIN = 1.1754943508222875e-38


def _tanh_dev(x):
    lib = _lib.load()
    y = x.clone()
    assert lib.hgt_tanh_inplace(y.data_ptr(), y.numel(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return y


def test_tanh_is_relative_accurate_at_every_magnitude():
    """hgt_tanh (hgt_split_common.h: the fused epilogues and hgt_tanh_inplace) against torch.tanh in float64 on +- log-spaced |x|
    from 1e-38 to 30, zeros, subnormals, infinities and NaN: relative error on normal inputs, absolute error, the sign (-0 too),
    exactly +-1 once saturated."""
    mag = torch.logspace(-38, math.log10(30.0), 200_001, dtype=torch.float64).float()
    special = torch.tensor([0.0, 1e-45, 3e-42, 1e-40, 5e-39, FLT_MIN, 0.25, 0.2499999, 0.2500001, 9.0, 9.1, 88.0, 3.4e38,
                            float("inf")], dtype=torch.float32)
    x = torch.cat([mag, -mag, special, -special, torch.tensor([float("nan"), -float("nan")])]).to(DEV)
    y = _tanh_dev(x)
    ref = torch.tanh(x.double())
    xa = x.abs()
    fin = torch.isfinite(x)
    normal = fin & (xa >= FLT_MIN)
    sub = fin & (xa < FLT_MIN) & (x != 0)
    err = (y.double() - ref).abs()
    rel = (err[normal] / ref[normal].abs()).max().item()
    absd = err[fin].max().item()
    worst_at = x[normal][(err[normal] / ref[normal].abs()).argmax()].item()
    print("\nhgt_tanh: max relative error %.2e (at x = %.6g), max absolute error %.2e over %d inputs" % (rel, worst_at, absd, x.numel()))
    assert rel <= TANH_REL_TOL
    assert absd <= TANH_ABS_TOL
    nn = ~torch.isnan(x)
    assert torch.equal(torch.signbit(y[nn]), torch.signbit(x[nn])), "sign lost (-0.0 included)"
    assert bool(((y[sub] == x[sub]) | (y[sub] == 0)).all())
    sat = fin & (xa >= 9.1)
    assert bool((y[sat] == torch.sign(x[sat])).all()), "not exactly +-1 once saturated"
    inf = torch.isinf(x)
    assert bool((y[inf] == torch.sign(x[inf])).all())
    assert bool(torch.isnan(y[torch.isnan(x)]).all())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1025, 1024 * 256 - 1, 1024 * 256 + 1, 1024 * 256 * 3 + 2])
def test_tanh_inplace_tail_and_launch_edges(n):
    """Every element of [0, n) is transformed, the element just past n is not (k_tanh_inplace: 4 per thread, 1024 per workgroup,
    a scalar tail loop)."""
    g = torch.Generator(device=DEV).manual_seed(n)
    buf = torch.empty(n + 8, device=DEV)
    v = (torch.rand(n, generator=g, device=DEV) * 2.5 + 0.5) * torch.where(torch.rand(n, generator=g, device=DEV) < 0.5, -1.0, 1.0)
    buf[:n] = v
    buf[n:] = 12345.0
    lib = _lib.load()
    assert lib.hgt_tanh_inplace(buf.data_ptr(), n, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    err = (buf[:n].double() - torch.tanh(v.double())).abs().max().item()
    print("\nhgt_tanh_inplace n=%d: max|err| %.2e, guard %s" % (n, err, buf[n].item()))
    assert err <= TANH_ABS_TOL
    assert bool((buf[n:] == 12345.0).all()), "written past n"


def test_tanh_inplace_rejects_a_pointer_that_is_not_16_byte_aligned():
    buf = torch.full((65,), 0.5, device=DEV)
    lib = _lib.load()
    assert lib.hgt_tanh_inplace(buf[1:].data_ptr(), 64, torch.cuda.current_stream().cuda_stream) == HGT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((buf == 0.5).all())


# ------------------------------------------------------------------ 3. the GNN stack on both sides of 65 536 nodes
SCHEMAS = {      # reference widths: ogbn-mag (gnn_mag4) and OAG (gnn_oag2), oracle/gen_golden_gnn.py
    "mag": dict(in_dim=129, n_hid=512, T=4, R=9, H=8, prev_norm=True, last_norm=True, sorted_types=True),
    "oag": dict(in_dim=1169, n_hid=400, T=5, R=33, H=8, prev_norm=False, last_norm=False, sorted_types=False),
}
GNN_CASES = [(s, n, 2, "f16x3") for s in ("mag", "oag") for n in (65_535, 65_536, 65_537)] + [
    ("oag", 65_535, 2, "bf16x3"),
    ("mag", 300_007, 4, "f16x3"),
]


def _taint(mask, ei, hops):
    """Rows whose value can depend on a row of `mask` within `hops` layers (out-neighbourhoods)."""
    m = mask.clone()
    for _ in range(hops):
        nxt = m.clone()
        nxt[ei[1][m[ei[0]]]] = True
        m = nxt
    return m


@pytest.mark.parametrize("schema,N,n_layers,precision", GNN_CASES, ids=["%s-%d-%dl-%s" % c for c in GNN_CASES])
def test_gnn_stack_at_full_graph_sizes_against_fp64(schema, N, n_layers, precision):
    """pyhgt_amd.GNN in eval mode at the reference widths, ~10 in-edges per node with a hub target, unclaimed edges and nodes of no
    known type, on both sides of the 65 536-node line (GNN.forward's adapter form, the plan's one-workgroup row lists, the item-
    parallel aggregation) and at 300k nodes.  Each stage on ~2000 check rows against float64, from the captured input of that
    stage: the adapter (unknown-type rows exactly 0), every layer (_fp64_rows).  The adapter's bits equal a plain typed linear +
    hgt_tanh_inplace, and a second forward is bit-identical outside the reach of the hub rows (fp32 atomics)."""
    from pyhgt_amd import GNN
    c = SCHEMAS[schema]
    in_dim, d, T, R, H = c["in_dim"], c["n_hid"], c["T"], c["R"], c["H"]
    f16 = precision == "f16x3"
    E = 10 * N
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, in_dim, T, R, seed=N % 1000 + in_dim, sorted_types=c["sorted_types"],
                                              strided_edge_index=False, device=DEV)
    hub = N // 3 + 17
    ei[1, :3000] = hub                                  # a hub target (> HGT_HUB_DEG in-edges)
    et[::17] = R + 2                                    # edges no relation claims
    nt[5::37] = T + 1                                   # nodes of no known type
    sd = O.make_gnn_state_dict(in_dim, d, T, R, H, n_layers, c["prev_norm"], c["last_norm"], True, seed=N % 13)
    gnn = GNN(in_dim, d, T, R, H, n_layers, 0.2, "hgt", c["prev_norm"], c["last_norm"], True).eval()
    gnn.load_state_dict(sd)
    gnn = gnn.to(DEV)
    for gc in gnn.gcs:
        gc.base_conv.precision = precision
    # the adapter's path: GNN.forward's switch, then typed_linear_split_impl with and without HGT_LINEAR_TANH
    asks = N < ADAPTER_EPILOGUE_MAX_N
    with_tanh = _split_dispatch(N, T, in_dim, d, int(in_dim % 4 == 0), tanh=True)
    epilogue = asks and with_tanh["kernel"] not in ("unsupported", "tile")
    plain = _split_dispatch(N, T, in_dim, d, int(in_dim % 4 == 0))
    pred = dict(asks_epilogue=asks, epilogue_ran=epilogue, plain_kernel=plain["kernel"], item_aggregation=N < ITEM_AGG_MAX_NODES,
                small_row_lists=(N <= SMALL_ROWS_N and T <= SMALL_ROWS_T))
    print("\n%s N=%d E=%d %d layers %s: %s, plain adapter %s" % (schema, N, E, n_layers, precision, pred, plain))
    assert epilogue == (N == 65_535 and in_dim == 1169)
    assert with_tanh["kernel"] == ("slab" if in_dim > KP else "unsupported")
    if epilogue:
        assert with_tanh["nstg"] == 2 and with_tanh["pass_split"] == 1
    captured = []
    hooks = [gnn.gcs[0].base_conv.register_forward_pre_hook(lambda m, a: captured.append(a[0].detach().clone()))]
    hooks += [gc.base_conv.register_forward_hook(lambda m, a, o: captured.append(o.detach().clone())) for gc in gnn.gcs]
    GraphPlan.clear_cache()
    poison = torch.full((N, d), float("nan"), device=DEV)      # (cached by the allocator: the adapter output may land on it)
    del poison
    with torch.no_grad():
        out = gnn(x, nt, tm, ei, et)
        torch.cuda.synchronize()
        for h in hooks[1:]:
            h.remove()
        out2 = gnn(x, nt, tm, ei, et)         # (its adapter output lands on memory the first forward left values in)
    torch.cuda.synchronize()
    hooks[0].remove()
    assert len(captured) == n_layers + 2
    assert torch.equal(captured.pop(), captured[0]), "the adapter of a second forward differs"
    assert bool(torch.isfinite(out).all())
    deg = torch.bincount(ei[1], minlength=N)
    tainted = _taint(deg > 1024, ei, n_layers)
    assert torch.equal(out[~tainted], out2[~tainted]), "a second forward differs outside the hub rows' reach"
    # check rows: type-boundary tiles, the highest in-degree rows, random rows (with every unknown-type row among them), the last tile
    tg = pick_check_targets(nt, ei[1], n_random=1800, seed=N % 7)
    tg = torch.unique(torch.cat([tg, torch.arange(max(0, N - 70), N, device=DEV), torch.tensor([hub], device=DEV)]))
    unknown = (nt[tg] < 0) | (nt[tg] >= T)
    assert int(unknown.sum()) > 0 and int(deg[tg].max()) > 1024
    # adapter vs float64
    h0 = captured[0]
    W = torch.stack([lin.weight.detach() for lin in gnn.adapt_ws]).float().contiguous()
    b = torch.stack([lin.bias.detach() for lin in gnn.adapt_ws]).float().contiguous()
    ref0 = torch.zeros(tg.numel(), d, dtype=torch.float64, device=DEV)
    for t in range(T):
        m = nt[tg] == t
        ref0[m] = torch.tanh(x[tg[m]].double() @ W[t].double().T + b[t].double())
    err0 = (h0[tg].double() - ref0).abs().max().item()
    assert bool((h0[tg[unknown]] == 0).all()), "rows of no known type must be exactly 0"
    assert bool((h0[(nt < 0) | (nt >= T)] == 0).all())
    # the adapter's bits: a plain typed linear on the plan's row lists + hgt_tanh_inplace
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rl = GraphPlan.cached(nt, ei, et, tm, T, R).row_lists()
    direct = torch.zeros(N, d, device=DEV)
    linear = lib.hgt_typed_linear_f16x3 if f16 else lib.hgt_typed_linear_bf16x3
    ws = _split_weights(W, f16)
    assert linear(x.data_ptr(), in_dim, rl.rows_all, rl.off_all, T, N, in_dim, d, ws.data_ptr(), b.data_ptr(), d, direct.data_ptr(),
                  None, None, d, 0, 0, st) == 0
    assert lib.hgt_tanh_inplace(direct.data_ptr(), direct.numel(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(h0, direct), "adapter differs from plain typed linear + hgt_tanh_inplace by %.3e" % (h0 - direct).abs().max()
    assert err0 < _gemm_tol(f16, in_dim), err0
    # every layer from its captured input
    g = dict(T=T, R=R, H=H, d=d, ids=torch.arange(N, device=DEV).unsqueeze(1), nt=nt, ei=ei, et=et, tm=tm, use_rte=True, deg=deg)
    errs = []
    for li in range(n_layers):
        pre = "gcs.%d.base_conv." % li
        lsd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        g["use_norm"] = c["prev_norm"] if li < n_layers - 1 else c["last_norm"]
        hin = captured[li]
        ref = _fp64_rows(lsd, g, tg, x_sub_of=lambda ids: hin[ids])
        errs.append((captured[li + 1][tg].double() - ref).abs().max().item())
    print("adapter max|err| %.2e (bound %.1e), layers %s (bound %.0e), %d check rows (%d of unknown type), %d rows in the hubs' reach"
          % (err0, _gemm_tol(f16, in_dim), ["%.2e" % e for e in errs], PREC_TOL[precision], tg.numel(), int(unknown.sum()),
             int(tainted.sum())))
    assert max(errs) < PREC_TOL[precision]
    GraphPlan.clear_cache()


# ------------------------------------------------------------------ 4. plan row lists on the 65 536 line
@pytest.mark.parametrize("N", [65_536, 65_537])
@pytest.mark.parametrize("T", [30, 31])
def test_plan_row_lists_at_the_one_workgroup_limit(N, T):
    """rows_all / off_all and the target lists rows_q / off_q (NQ < N: halo rows) against numpy stable argsorts of the type
    bucket, with node types that are negative, equal to T or far above it: the one-workgroup kernel with s_key[65536] full, and
    the radix sorts one node or one type beyond it."""
    R, NQ = 4, N - 1001
    g = torch.Generator().manual_seed(N + T)
    nt = torch.randint(0, T, (N,), generator=g)
    nt[::97] = -1
    nt[3::101] = -(1 << 40)
    nt[5::89] = T
    nt[7::83] = T + 1000
    nt[-1] = 1 << 40
    E = 300_000
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, NQ, (E,), generator=g)])
    et = torch.randint(0, R, (E,), generator=g)
    small = N <= SMALL_ROWS_N and T <= SMALL_ROWS_T
    print("\nN=%d NQ=%d T=%d: one-workgroup row lists %s" % (N, NQ, T, small))
    assert small == (N == 65_536 and T == 30)
    plan = GraphPlan(*_to_dev(nt, ei, et), None, T, R, n_q_rows=NQ)
    torch.cuda.synchronize()
    p = _plan_arrays(plan)
    assert p["bad"] == 0
    key = np.where((nt.numpy() >= 0) & (nt.numpy() < T), nt.numpy(), T)
    for rows, off, n in ((p["rows_all"], p["off_all"], N), (p["rows_q"], p["off_q"], NQ)):
        k = key[:n]
        assert np.array_equal(rows[:n], np.argsort(k, kind="stable").astype(np.int32))
        assert np.array_equal(off, np.searchsorted(np.sort(k), np.arange(T + 2)).astype(np.int32))


# ------------------------------------------------------------------ 5. heads at real shapes
def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("n_out", [1, 63, 65, 349, 4099])
@pytest.mark.parametrize("n_hid", [400, 512])
def test_classifier_at_real_shapes(n_hid, n_out):
    """Classifier (hgt_typed_linear + hgt_log_softmax_rows) at 1, 3, 5 and 100 003 rows against float64; every 7th row has its
    logits spread over +-1e4 (inputs scaled): finite, within 1e-5 of |value| or of the row's logit scale."""
    from pyhgt_amd import Classifier
    torch.manual_seed(n_hid + n_out)
    clf = Classifier(n_hid, n_out).eval().to(DEV)
    n = 100_003
    gd = torch.Generator(device=DEV).manual_seed(n_out)
    x = torch.randn(n, n_hid, generator=gd, device=DEV)
    spread = torch.zeros(n, dtype=torch.bool, device=DEV)
    spread[::7] = True
    x[spread] *= 6000.0
    W, bb = clf.linear.weight.detach().double(), clf.linear.bias.detach().double()
    for rows in (1, 3, 5, n):
        with torch.no_grad():
            out = clf(x[:rows]).reshape(rows, n_out)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        worst, worst_spread, span = 0.0, 0.0, 0.0
        for lo in range(0, rows, 16384):
            sl = slice(lo, min(rows, lo + 16384))
            logits = x[sl].double() @ W.T + bb
            ref = torch.log_softmax(logits, dim=-1)
            scale = torch.where(spread[sl, None], logits.abs().amax(1, keepdim=True), torch.ones_like(logits[:, :1]))
            e = (out[sl].double() - ref).abs() / torch.maximum(ref.abs(), scale).clamp(min=1.0)
            worst = max(worst, e[~spread[sl]].max().item() if bool((~spread[sl]).any()) else 0.0)
            worst_spread = max(worst_spread, e[spread[sl]].max().item() if bool(spread[sl].any()) else 0.0)
            span = max(span, (logits.amax(1) - logits.amin(1)).max().item())
        print("Classifier(%d, %d) rows=%d: relative error %.2e, spread rows %.2e (logit span %.0f)" % (n_hid, n_out, rows, worst,
                                                                                                      worst_spread, span))
        assert worst < 1e-5 and worst_spread < 1e-5
        if rows == n and n_out > 1:
            assert span > 1e4


@pytest.mark.parametrize("n_hid", [400, 512])
def test_matcher_at_real_shapes(n_hid):
    """Matcher: pair=True (hgt_row_dot) on 10 001 rows, all pairs of 10 000 x 2 003 candidates (the typed linear with y as a
    2003-row weight and no bias), and the inference cache, against float64."""
    from pyhgt_amd import Matcher
    torch.manual_seed(n_hid)
    mt = Matcher(n_hid).eval().to(DEV)
    gd = torch.Generator(device=DEV).manual_seed(n_hid)
    xp, yp = torch.randn(10_001, n_hid, generator=gd, device=DEV), torch.randn(10_001, n_hid, generator=gd, device=DEV)
    x, y, y2 = (torch.randn(10_000, n_hid, generator=gd, device=DEV), torch.randn(2003, n_hid, generator=gd, device=DEV),
                torch.randn(2003, n_hid, generator=gd, device=DEV))
    Wl, bl = mt.left_linear.weight.detach().double(), mt.left_linear.bias.detach().double()
    Wr, br = mt.right_linear.weight.detach().double(), mt.right_linear.bias.detach().double()
    s = n_hid ** 0.5
    with torch.no_grad():
        pair = mt(xp, yp, pair=True)
        full = mt(x, y)
        cached = mt(x, y, infer=True)
        cached2 = mt(torch.zeros_like(x), y2, infer=True)     # tx from the cache, ty from y2
    torch.cuda.synchronize()
    tx = x.double() @ Wl.T + bl
    e_pair = _rel(pair, ((xp.double() @ Wl.T + bl) * (yp.double() @ Wr.T + br)).sum(-1) / s)
    e_full = _rel(full, tx @ (y.double() @ Wr.T + br).T / s)
    e_c2 = _rel(cached2, tx @ (y2.double() @ Wr.T + br).T / s)
    print("\nMatcher(%d): pair %.2e, all pairs %.2e, cached %.2e" % (n_hid, e_pair, e_full, e_c2))
    assert pair.shape == (10_001,) and full.shape == (10_000, 2003)
    assert e_pair < 1e-5 and e_full < 1e-5 and e_c2 < 1e-5
    assert torch.equal(cached, full)


def _grads_vs_fp64(mod, inputs, fwd, seed):
    """Gradients of <fwd(mod, *inputs), G> (G random) for every parameter and input, against a float64 copy under torch autograd."""
    ins = [t.clone().requires_grad_(True) for t in inputs]
    out = fwd(mod, *ins)
    gout = torch.randn(out.shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)
    (out * gout).sum().backward()
    params = dict(mod.named_parameters())
    ref_p = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    ins64 = [t.detach().double().clone().requires_grad_(True) for t in inputs]
    out64 = fwd_fp64(mod, ref_p, *ins64)
    (out64 * gout.double()).sum().backward()
    errs = {"out": _rel(out.detach(), out64.detach())}
    for k, v in params.items():
        errs[k] = _rel(v.grad, ref_p[k].grad)
    for i, (a, r) in enumerate(zip(ins, ins64)):
        errs["d_in%d" % i] = _rel(a.grad, r.grad)
    return errs


def fwd_fp64(mod, p, *ins):
    from pyhgt_amd import Classifier
    lin = torch.nn.functional.linear
    if isinstance(mod, Classifier):
        return torch.log_softmax(lin(ins[0], p["linear.weight"], p["linear.bias"]), dim=-1)
    tx = lin(ins[0], p["left_linear.weight"], p["left_linear.bias"])
    ty = lin(ins[1], p["right_linear.weight"], p["right_linear.bias"])
    if mod._pair:
        return (tx * ty).sum(-1) / mod.sqrt_hd
    return tx @ ty.T / mod.sqrt_hd


@pytest.mark.parametrize("head", ["classifier-349", "classifier-4099", "matcher-pair", "matcher-all-pairs"])
@pytest.mark.parametrize("n_hid", [400, 512])
def test_head_gradients_against_fp64(head, n_hid):
    """Training mode: the gradients of every parameter and of both inputs through TypedLinearFunction (typed weight gradient,
    column sums, input gradient), incl. the all-pairs Matcher whose candidate projection is the typed linear's WEIGHT (no bias,
    2003 rows: not a multiple of 4)."""
    from pyhgt_amd import Classifier, Matcher
    torch.manual_seed(n_hid + len(head))
    gd = torch.Generator(device=DEV).manual_seed(n_hid)
    if head.startswith("classifier"):
        mod = Classifier(n_hid, int(head.split("-")[1])).train().to(DEV)
        inputs = [torch.randn(1003, n_hid, generator=gd, device=DEV)]
        fwd = lambda m, x: m(x)       # noqa: E731
    else:
        mod = Matcher(n_hid).train().to(DEV)
        mod._pair = head == "matcher-pair"
        n_y = 3001 if mod._pair else 2003
        inputs = [torch.randn(3001, n_hid, generator=gd, device=DEV), torch.randn(n_y, n_hid, generator=gd, device=DEV)]
        fwd = lambda m, x, y: m(x, y, pair=m._pair)     # noqa: E731
    errs = _grads_vs_fp64(mod, inputs, fwd, seed=n_hid)
    print("\n%s n_hid=%d: relative errors %s" % (head, n_hid, {k: "%.1e" % v for k, v in errs.items()}))
    assert len(errs) == 1 + len(list(mod.parameters())) + len(inputs)
    assert max(errs.values()) < 1e-5
