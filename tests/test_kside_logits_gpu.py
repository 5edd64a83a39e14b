"""hgt_edge_logits_kside: attention logits with the relation transform applied to the K row of every edge on the matrix cores
(csrc/hgt_edge_logits_kside.hip).  Whole layers with the kernel forced (kernel_flags = 65536) against the fp64 closed form on
every batch shape it has -- ragged, full, double-buffered, padded d_k, padded heads, a single edge, no edge --, its scale rule at
extreme magnitudes, bit-reproducibility, and the shapes it does not cover."""
import ctypes as C

import pytest
import torch

from oracle import hgt_oracle as O
from pyhgt_amd import HGTConv, GraphPlan, _lib
from pyhgt_amd.synth import synthetic_typed_graph

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
def _direct_setup(N, E, d, H, T, R, x_scale, seed):
    """Q, K (fp64 typed linears of x * x_scale, rounded to fp32: LayerNorm plays no part), the packed relation matrices and the plan
    of a graph with unclaimed edges, on the device; d_k = 32 and H a power of two (no padding anywhere)."""
    lib = _lib.load()
    dk = d // H
    assert dk == 32
    sd = O.make_state_dict(d, d, T, R, H, False, False, seed=seed)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=seed + 1)
    et = et.clone()
    et[::41] = R
    xs = x.double() * x_scale
    Q = torch.zeros(N, d, dtype=torch.float64)
    K = torch.zeros(N, d, dtype=torch.float64)
    for t in range(T):
        m = nt == t
        Q[m] = xs[m] @ sd["q_linears.%d.weight" % t].double().T + sd["q_linears.%d.bias" % t].double()
        K[m] = xs[m] @ sd["k_linears.%d.weight" % t].double().T + sd["k_linears.%d.bias" % t].double()
    Qd, Kd = Q.float().to(DEV).contiguous(), K.float().to(DEV).contiguous()
    ra, rm, rp = (sd[k].float().to(DEV).contiguous() for k in ("relation_att", "relation_msg", "relation_pri"))
    att_t = torch.empty(R * H * dk * dk, dtype=torch.float32, device=DEV)
    msg_p = torch.empty_like(att_t)
    assert lib.hgt_relation_pack(ra.data_ptr(), rm.data_ptr(), rp.data_ptr(), R, H, H, dk, dk, att_t.data_ptr(), msg_p.data_ptr(), _st()) == 0
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


def _logits_fp64(s):
    """fp64 logits of the kernel's own fp32 inputs, and sum |q| |A'| |k| per (edge, head): the scale of their rounding errors"""
    E, H, R, dk = s["E"], s["H"], s["R"], s["dk"]
    Q, K = s["Q"].cpu().double().view(-1, H, dk), s["K"].cpu().double().view(-1, H, dk)
    A = s["att_t"].cpu().double().view(R, H, dk, dk)          # [r][h][output j][k c]
    src, dst, et = s["ei"][0], s["ei"][1], s["et"]
    ref = torch.zeros(E, H, dtype=torch.float64)
    mag = torch.zeros(E, H, dtype=torch.float64)
    for r in range(R):
        sel = (et == r).nonzero().flatten()
        k, q = K[src[sel]].transpose(0, 1), Q[dst[sel]].transpose(0, 1)          # [h][e][dk]
        ref[sel] = (torch.bmm(k, A[r].transpose(1, 2)) * q).sum(-1).T
        mag[sel] = (torch.bmm(k.abs(), A[r].abs().transpose(1, 2)) * q.abs()).sum(-1).T
    return ref, mag


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
