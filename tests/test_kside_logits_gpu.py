"""hgt_edge_logits_kside: attention logits with the relation transform applied to the K row of every edge on the matrix cores
(csrc/hgt_edge_logits_kside.hip).  Whole layers with the kernel forced (kernel_flags = 65536) against the fp64 closed form on
every batch shape it has -- ragged, full, double-buffered, padded d_k, padded heads, a single edge, no edge --, its scale rule at
extreme magnitudes, bit-reproducibility, and the shapes it does not cover.

The kernel's own edges go through the entry point (hgt_edge_logits_kside) at H = 2, 4 and 8, on the input sets of
test_kside_scale_rule.py (which shows, without a GPU, that the quantisation of the scale rule alone stays below half the bound on
each of them: 0.002 .. 0.010 of it).  Bound everywhere: |error| <= 2^-17 sum |q| |A'| |k| per (edge, head), plus 2^-149 where the
fp64 logit is below fp32's normal range.  Measured worst error / bound on an MI355X:
  uniform magnitudes, x * 2^0 / 2^20 / 2^-20 (H = 8, 32-edge items)                       0.006 / 0.005 / 0.006
  uneven rows (exponents per row and block, zero / half / dominant / subnormal rows),
    64-edge items, H = 2 / 4 / 8, logits in fp32's normal range                           0.012 / 0.020 / 0.021
    ... logits that round to fp32 subnormals (half a step of 2^-149 against the 2^-149)   0.498 / 0.492 / 0.498
  512-edge items, 16 batches per item (H = 8, E = 2 097 152)                              0.0059
  rows 2.25 GB from the base of Q and K (N = 2 200 000), and the same graph on 8192 rows  0.0050, bit-identical
One inf in K and one NaN in Q make exactly the 1766 logits of their (edges, head) non-finite; the others keep their bits."""
import ctypes as C

import pytest
import torch

from oracle import hgt_oracle as O
from pyhgt_amd import HGTConv, GraphPlan, _lib
from pyhgt_amd.synth import synthetic_typed_graph
import test_kside_scale_rule as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
F16_TOL = 1e-5
PREC_TOL = {"bf16x3": TOL, "f16x3": F16_TOL}          # the bounds of tests/test_hgt_gpu.py
ATT_TOL = {"bf16x3": 1e-5, "f16x3": 2e-6}
KSIDE, NO_KSIDE = 65536, 131072                       # HGT_FLAG_KSIDE_LOGITS, HGT_FLAG_NO_KSIDE_LOGITS
UNSUPPORTED = -2


def _st():
    return torch.cuda.current_stream().cuda_stream


def _layer(sd, d, T, R, H, use_RTE, precision, use_norm=True):
    layer = HGTConv(d, d, T, R, H, 0.2, use_norm, use_RTE, keep_att=True, precision=precision).eval()
    layer.load_state_dict(sd)
    return layer.to(DEV)


def _run(layer, x, nt, ei, et, tm, flags):
    layer.kernel_flags = flags
    GraphPlan.clear_cache()
    with torch.no_grad():
        out = layer(*[None if t is None else t.to(DEV) for t in (x, nt, ei, et, tm)])
    torch.cuda.synchronize()
    return out.cpu(), layer.att.cpu()


CASES = [
    # N, E, d, H, T, R, also with the default route
    (3000, 30000, 256, 8, 4, 8, False),       # the benchmark layout; 16-edge items: every batch is ragged
    (600, 150000, 256, 8, 3, 4, False),       # 32-edge items: full batches, one per item (in-degree ~250: no hubs)
    (400, 270000, 64, 2, 2, 3, True),         # 64-edge items: two or more batches per item -- the double-buffered loop at the default route's own item size
    (700, 3000, 32, 2, 3, 2, False),          # d_k = 16 padded to 32
    (500, 4000, 96, 3, 2, 3, False),          # three heads running as four: one padded head
    (129, 1, 256, 8, 2, 2, False),            # a single edge
]
_shared = {}


def _case(case):
    """graph, weights and the fp64 reference of a case: computed once, shared by the precisions, never modified"""
    if case not in _shared:
        N, E, d, H, T, R, _ = case
        sd = O.make_state_dict(d, d, T, R, H, True, False, seed=N + E + d)
        x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=E + 7)
        et = et.clone()
        et[::41] = R                          # unclaimed edges: logit 0
        ref, att_ref = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, use_norm=True, use_RTE=False, dtype=torch.float64,
                                             return_att=True)
        _shared[case] = (sd, x, nt, ei, et, ref, att_ref)
    return _shared[case]


@pytest.mark.parametrize("precision", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_layer_with_kside_logits_matches_the_closed_form(case, precision):
    N, E, d, H, T, R, default_too = case
    sd, x, nt, ei, et, ref, att_ref = _case(case)
    layer = _layer(sd, d, T, R, H, False, precision)
    out, att = _run(layer, x, nt, ei, et, None, KSIDE)
    err, err_att = (out.double() - ref).abs().max().item(), (att.double() - att_ref).abs().max().item()
    print("kside logits N=%d E=%d d=%d H=%d %s: max|out| err %.2e, att err %.2e" % (N, E, d, H, precision, err, err_att))
    assert err < PREC_TOL[precision]
    assert err_att < ATT_TOL[precision]
    out2, att2 = _run(layer, x, nt, ei, et, None, NO_KSIDE)      # the vector-ALU kernel
    d_att = (att2 - att).abs().max().item()
    print("   against the vector-ALU kernel: att diff %.2e" % d_att)
    assert d_att < 1e-5
    if default_too:
        out3, att3 = _run(layer, x, nt, ei, et, None, 0)
        err3, err_att3 = (out3.double() - ref).abs().max().item(), (att3.double() - att_ref).abs().max().item()
        print("   default route: max|out| err %.2e, att err %.2e" % (err3, err_att3))
        assert err3 < PREC_TOL[precision] and err_att3 < ATT_TOL[precision]
        assert (att2 - att3).abs().max().item() < 1e-5


@pytest.mark.parametrize("precision", ["bf16x3", "f16x3"])
def test_edgeless_graph(precision):
    N, d, H, T, R = 300, 256, 8, 3, 4
    sd = O.make_state_dict(d, d, T, R, H, True, False, seed=3)
    x, nt, ei, et, tm = synthetic_typed_graph(N, 10, d, T, R, seed=4)
    ei, et = ei[:, :0].contiguous(), et[:0].contiguous()
    layer = _layer(sd, d, T, R, H, False, precision)
    out, _ = _run(layer, x, nt, ei, et, None, KSIDE)
    out2, _ = _run(layer, x, nt, ei, et, None, NO_KSIDE)
    assert torch.isfinite(out).all() and torch.equal(out, out2)


# ------------------------------------------------------------------ the entry point itself
def _direct_setup(N, E, d, H, T, R, x_scale, seed, inputs=None):
    """Q, K (fp64 typed linears of x * x_scale, rounded to fp32: LayerNorm plays no part), the packed relation matrices and the plan
    of a graph with unclaimed edges, on the device; d_k = 32 and H in {2, 4, 8} (no padding anywhere).  inputs: an input set of
    test_kside_scale_rule.py instead -- its Q and K as they are (edited rows and all; tensors on either device), its edits of
    att_t applied to what hgt_relation_pack wrote, in front of hgt_relation_kside_pack; N may exceed the set's rows if Q / K do."""
    lib = _lib.load()
    dk = d // H
    assert dk == 32 and H in (2, 4, 8)
    inp = inputs if inputs is not None else S.plain_inputs(N, E, H, T, R, seed, x_scale)
    assert (inp["E"], inp["H"], inp["T"], inp["R"]) == (E, H, T, R)
    sd, nt, ei, et = inp["sd"], inp["nt"], inp["ei"], inp["et"]
    Qd, Kd = inp["Q"].to(DEV).contiguous(), inp["K"].to(DEV).contiguous()
    assert Qd.shape == (N, d) and Kd.shape == (N, d) and Qd.dtype == torch.float32 and nt.numel() == N and int(ei.max()) < N
    ra, rm, rp = (sd[k].float().to(DEV).contiguous() for k in ("relation_att", "relation_msg", "relation_pri"))
    att_t = torch.empty(R * H * dk * dk, dtype=torch.float32, device=DEV)
    msg_p = torch.empty_like(att_t)
    assert lib.hgt_relation_pack(ra.data_ptr(), rm.data_ptr(), rp.data_ptr(), R, H, H, dk, dk, att_t.data_ptr(), msg_p.data_ptr(), _st()) == 0
    att_t = S.edit_att(inp, att_t.view(R, H, dk, dk)).view(-1)
    nb = C.c_uint64()
    assert lib.hgt_relation_kside_bytes(R, H, dk, C.byref(nb)) == 0 and nb.value > 0
    img = torch.empty(int(nb.value), dtype=torch.uint8, device=DEV)
    assert lib.hgt_relation_kside_pack(att_t.data_ptr(), R, H, dk, img.data_ptr(), _st()) == 0
    plan = GraphPlan(nt.to(DEV), ei.to(DEV), et.to(DEV), None, T, R)
    return dict(lib=lib, plan=plan, Q=Qd, K=Kd, att_t=att_t, img=img, ei=ei, et=et, N=N, E=E, H=H, T=T, R=R, dk=dk)


def _direct_logits(s):
    """hgt_edge_logits_kside -> logits by edge id [E][H]"""
    lib, plan, E, H, T, R = s["lib"], s["plan"], s["E"], s["H"], s["T"], s["R"]
    srt = torch.full((E, H), float("nan"), dtype=torch.float32, device=DEV)
    rc = lib.hgt_edge_logits_kside(plan.ptr, plan.N, E, T, R, H, s["dk"], s["Q"].data_ptr(), s["K"].data_ptr(), None, s["att_t"].data_ptr(),
                                   s["img"].data_ptr(), 1, srt.data_ptr(), _st())
    assert rc == 0
    out = torch.empty_like(srt)
    assert lib.hgt_att_export(plan.ptr, plan.N, E, T, R, H, srt.data_ptr(), out.data_ptr(), H, _st()) == 0
    torch.cuda.synchronize()
    return out.cpu()


def _logits_fp64(s, on_device=False):
    """fp64 logits of the kernel's own fp32 inputs, and sum |q| |A'| |k| per (edge, head): the scale of their rounding errors.
    on_device: the same float64 sums computed there (graphs of 262 144 edges and more)."""
    Q, K = (s["Q"], s["K"]) if on_device else (s["Q"].cpu(), s["K"].cpu())
    ref, mag = S.logits_fp64(Q, K, s["att_t"], s["ei"], s["et"], s["R"], s["H"])
    return ref.cpu(), mag.cpu()


def _item_edges(lib, E):
    ce = C.c_int32()
    assert lib.hgt_plan_item_edges(E, C.byref(ce)) == 0
    return ce.value


def _against_bound(got, ref, mag, what):
    """|error| <= 2^-17 sum |q| |A'| |k| per (edge, head), plus one fp32 subnormal step where the fp64 value is below fp32's normal
    range (the final ldexp rounds there); prints and returns the worst error / bound."""
    err = (got.double() - ref).abs()
    bound = 2.0 ** -17 * mag + (ref.abs() < 2.0 ** -126).double() * 2.0 ** -149
    ratio = err / bound.clamp(min=1e-300)
    worst = ratio.max().item()
    normal = ref.abs() >= 2.0 ** -126
    print("%s: worst err / bound %.4f at (edge, head) %s; %.4f over the %d logits in fp32's normal range" % (
        what, worst, divmod(int(ratio.argmax()), got.shape[1]), ratio[normal].max().item(), int(normal.sum())))
    assert bool((err <= bound).all()), worst
    return worst


@pytest.mark.parametrize("log2_scale", [0, 20, -20])
def test_scale_rule_at_extreme_magnitudes(log2_scale):
    """The second case with x scaled by 2^20 and 2^-20 (Q and K carry the scale: logits of ~2^40 and ~2^-40 times the usual).
    Bound: the kernel sums 96 fp16 x fp16 products per output and 32 fp32 products per logit in fp32 -- at most ~130 roundings of
    2^-24 relative to the sum of magnitudes -- over operands split to 2^-22: |error| <= 2^-17 sum |q| |A'| |k|, whatever the scale,
    and nothing may overflow or vanish."""
    s = _direct_setup(600, 150000, 256, 8, 3, 4, 2.0 ** log2_scale, seed=21)
    got = _direct_logits(s)
    assert torch.isfinite(got).all(), "inf / NaN in the logits"
    ref, mag = _logits_fp64(s)
    err = (got.double() - ref).abs()
    top = ref.abs().max().item()
    print("kside logits x * 2^%d: largest logit %.3e, max err / largest logit %.2e, max err / bound %.3f"
          % (log2_scale, top, err.max().item() / top, (err / (2.0 ** -17 * mag + 1e-300)).max().item()))
    assert top > 0 and (got[s["et"] == s["R"]] == 0).all()
    assert (err <= 2.0 ** -17 * mag).all()
    assert err.max().item() / top < 2.0 ** -17 * (mag.max().item() / top)


def test_two_runs_are_bit_identical():
    s = _direct_setup(600, 150000, 256, 8, 3, 4, 1.0, seed=21)
    a, b = _direct_logits(s), _direct_logits(s)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("precision", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("what", ["temporal", "dk64"])
def test_uncovered_layers_take_the_present_kernels(what, precision):
    """Temporal encoding and d_k = 64 with the force flag set: the layer silently runs the kernels it ran before, same bounds."""
    N, E, d, H, T, R = (1500, 12000, 256, 8, 3, 5) if what == "temporal" else (1200, 9000, 256, 4, 2, 4)
    use_RTE = what == "temporal"
    sd = O.make_state_dict(d, d, T, R, H, True, use_RTE, seed=N + E)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=E + 7)
    et = et.clone()
    et[::41] = R
    ref, att_ref = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, use_norm=True, use_RTE=use_RTE, dtype=torch.float64, return_att=True)
    layer = _layer(sd, d, T, R, H, use_RTE, precision)
    out, att = _run(layer, x, nt, ei, et, tm if use_RTE else None, KSIDE)
    assert (out.double() - ref).abs().max().item() < PREC_TOL[precision]
    assert (att.double() - att_ref).abs().max().item() < ATT_TOL[precision]
    out2, att2 = _run(layer, x, nt, ei, et, tm if use_RTE else None, NO_KSIDE)
    assert torch.equal(att, att2) and torch.equal(out, out2)


def test_entry_point_refuses_what_it_does_not_cover():
    s = _direct_setup(300, 2000, 256, 8, 2, 3, 1.0, seed=5)
    lib, plan = s["lib"], s["plan"]
    srt = torch.zeros(s["E"], 8, dtype=torch.float32, device=DEV)
    args = lambda H, dkp, rte: (plan.ptr, plan.N, s["E"], s["T"], s["R"], H, dkp, s["Q"].data_ptr(), s["K"].data_ptr(), rte,
                                s["att_t"].data_ptr(), s["img"].data_ptr(), 1, srt.data_ptr(), _st())
    assert lib.hgt_edge_logits_kside(*args(8, 32, s["K"].data_ptr())) == UNSUPPORTED      # temporal rows
    assert lib.hgt_edge_logits_kside(*args(4, 64, None)) == UNSUPPORTED                    # d_k = 64
    assert lib.hgt_edge_logits_kside(*args(8, 32, None)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the kernel's own edges (input sets: test_kside_scale_rule.py)
@pytest.mark.parametrize("H", [2, 4, 8])
def test_scale_rule_on_uneven_rows(H):
    """Every (row, head) of Q and K and every (relation, head) block of att_t at an exponent of its own (2^-40 .. 2^40, blocks
    2^-30 .. 2^30), zero rows and a zero block, rows whose halves or one element differ by 2^20 (the cross-half maximum), a
    subnormal K row, a Q row at 2^120: 64-edge items, so every head count runs several batches per item with ragged tails (H = 4, 8:
    the four-head pipeline).  A scale taken from the wrong operand, half or columns, or a wrong clamp, leaves the bound here; at
    uniform magnitudes it would not."""
    inp = S.uneven_inputs(H)
    s = _direct_setup(inp["N"], inp["E"], 32 * H, H, inp["T"], inp["R"], 1.0, 0, inputs=inp)
    assert _item_edges(s["lib"], s["E"]) == 64
    n_special = S.special_edge_counts(inp)
    assert min(n_special.values()) >= 32, n_special
    assert torch.equal(s["att_t"].cpu().view(-1) == 0, inp["att_t"].view(-1) == 0)
    got = _direct_logits(s)
    assert torch.isfinite(got).all(), "inf / NaN in the logits"
    ref, mag = _logits_fp64(s, on_device=True)
    assert float(ref.abs().max()) < 2.0 ** 126 and float(ref.abs().max()) > 2.0 ** 60
    _against_bound(got, ref, mag, "kside logits, uneven rows, H = %d (%s)" % (H, n_special))
    zero = S.zero_logit_mask(inp)
    assert int(zero.sum()) > s["E"] // 41 and bool((got[zero] == 0).all()), "logits of unclaimed edges, zero rows and the zero block must be exactly 0"
    assert bool((got[s["et"] == s["R"]] == 0).all())
    # the special rows one by one: their worst error / bound is reported with them
    src, dst = s["ei"][0], s["ei"][1]
    for name, (what, idx, h) in inp["special"].items():
        m = ((src == idx) if what == "K" else (dst == idx) if what == "Q" else (s["et"] == idx)) & (s["et"] < s["R"])
        e, b = (got[m, h].double() - ref[m, h]).abs(), 2.0 ** -17 * mag[m, h] + (ref[m, h].abs() < 2.0 ** -126).double() * 2.0 ** -149
        print("   %-18s %5d edges, head %d: worst err / bound %.4f, largest |logit| %.3e" % (
            name, int(m.sum()), h, (e / b.clamp(min=1e-300)).max().item(), ref[m, h].abs().max().item()))
    pair = (src == 18) & (dst == 19) & (s["et"] < s["R"])
    assert bool((ref[pair, inp["special"]["k_subnormal"][2]] != 0).any()) and bool((got[pair, inp["special"]["k_subnormal"][2]] != 0).any())


def test_many_batches_per_item():
    """512-edge items: 16 batches per item and wavefront -- the pipeline's steady state (pieces three steps ahead, edge indices one
    batch further) at H = 8, as the benchmark runs it, through the entry point."""
    inp = S.many_batches_inputs()
    s = _direct_setup(inp["N"], inp["E"], 256, 8, inp["T"], inp["R"], 1.0, 0, inputs=inp)
    assert _item_edges(s["lib"], s["E"]) == 512
    got = _direct_logits(s)
    assert torch.isfinite(got).all()
    ref, mag = _logits_fp64(s, on_device=True)
    _against_bound(got, ref, mag, "kside logits, 512-edge items")
    assert float(ref.abs().max()) > 0 and bool((got[s["et"] == s["R"]] == 0).all())


def test_non_finite_inputs_stay_where_they_are():
    """One inf in K and one NaN in Q: exactly the logits of (edges out of that source, that head) and (edges into that target, that
    head) are non-finite, every other logit has the bits of the run without the two values -- an edge is a column of the matrix
    product, and a clamped or re-read row of another lane must not leak."""
    H = 4
    inp = S.plain_inputs(300, 270000, H, 2, 3, seed=44)
    s = _direct_setup(inp["N"], inp["E"], 32 * H, H, inp["T"], inp["R"], 1.0, 0, inputs=inp)
    clean = _direct_logits(s)
    assert torch.isfinite(clean).all()
    j, hk, i, hq = 37, 1, 211, 2
    s["K"].view(-1, H, 32)[j, hk, 9] = float("inf")
    s["Q"].view(-1, H, 32)[i, hq, 27] = float("nan")
    got = _direct_logits(s)
    claimed = s["et"] < s["R"]
    want = torch.zeros(s["E"], H, dtype=torch.bool)
    want[:, hk] |= (s["ei"][0] == j) & claimed
    want[:, hq] |= (s["ei"][1] == i) & claimed
    assert int(want[:, hk].sum()) >= 32 and int(want[:, hq].sum()) >= 32
    bad = ~torch.isfinite(got)
    print("non-finite inputs: %d logits expected non-finite, %d are; %d of them unexpected, %d missing"
          % (int(want.sum()), int(bad.sum()), int((bad & ~want).sum()), int((want & ~bad).sum())))
    assert torch.equal(bad, want)
    assert torch.equal(got.view(torch.int32)[~want], clean.view(torch.int32)[~want])


def test_rows_between_2_and_4_gib_from_the_base():
    """2 200 000 rows of 1024 bytes: the last 4096 sit 2.25 GB from the bases of Q and K, where the 32-bit lane offsets and the
    record count of the buffer descriptors have their top bit set.  60 000 edges among the first and the last 4096 rows (both
    directions across the 2 GiB mark), bit-identical to the same graph renumbered onto 8192 rows, and within the bound."""
    if torch.cuda.get_device_properties(0).total_memory < 16 << 30:
        pytest.skip("two tables of 2.25 GB and their plan need a GPU with 16 GiB or more")
    small = S.far_rows_inputs()
    n_s, half, N, H = small["N"], small["N"] // 2, 2_200_000, 8
    assert (N - half) * 1024 > 1 << 31 and N * 1024 < 1 << 32
    s_small = _direct_setup(n_s, small["E"], 256, H, small["T"], small["R"], 1.0, 0, inputs=small)
    got_small = _direct_logits(s_small)
    ref, mag = _logits_fp64(s_small)
    _against_bound(got_small, ref, mag, "kside logits, 8192 rows")
    far = lambda v: torch.where(v < half, v, v + (N - n_s))
    big = dict(small, N=N, ei=far(small["ei"]))
    big["nt"] = torch.cat([small["nt"][:half], small["nt"][half:half + 1].expand(N - n_s), small["nt"][half:]])
    for k in ("Q", "K"):
        t = torch.zeros(N, 256, dtype=torch.float32, device=DEV)
        t[:half], t[N - half:] = small[k][:half].to(DEV), small[k][half:].to(DEV)
        big[k] = t
    src, dst = big["ei"][0], big["ei"][1]
    assert int(((src < half) & (dst >= N - half)).sum()) > 10000 and int(((src >= N - half) & (dst < half)).sum()) > 10000
    s_big = _direct_setup(N, small["E"], 256, H, small["T"], small["R"], 1.0, 0, inputs=big)
    got = _direct_logits(s_big)
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0
    _against_bound(got, ref, mag, "kside logits, rows 2.25 GB from the base")
    n_diff = int((got.view(torch.int32) != got_small.view(torch.int32)).sum())
    assert n_diff == 0, "%d logits differ from the renumbered graph" % n_diff
