"""hgt_edge_logits_kside, gather of K[src] and Q[dst] in whole head lines through LDS (the default form) against the per-lane
gather it replaces (HGT_FLAG_KSIDE_LANE_GATHER): the arithmetic is the same, so whole layers with the kernel forced
(HGT_FLAG_KSIDE_LOGITS, keep_att) must agree BIT FOR BIT on the output and on the attention weights, in both split precisions, on
the smallest shapes at which a gather can go wrong -- partly clamped pieces, partly filled batches, many batches per item,
unclaimed items between claimed ones, H = 2 / 4 / 8, identical lines inside a piece, sources at the end of the table -- and the
first three graphs also agree with the fp64 closed form within the bounds of test_kside_logits_gpu.py."""
import pytest
import torch

from oracle import hgt_oracle as O
from pyhgt_amd import HGTConv, GraphPlan, _lib
from pyhgt_amd.synth import synthetic_typed_graph
from test_kside_logits_gpu import PREC_TOL, ATT_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KSIDE = _lib.HGT_FLAG_KSIDE_LOGITS
LANE = _lib.HGT_FLAG_KSIDE_LOGITS | _lib.HGT_FLAG_KSIDE_LANE_GATHER
PRECISIONS = ["bf16x3", "f16x3"]


def _layer(sd, d, T, R, H, precision):
    layer = HGTConv(d, d, T, R, H, 0.2, True, False, keep_att=True, precision=precision).eval()
    layer.load_state_dict(sd)
    return layer.to(DEV)


def _run(layer, graph, flags):
    layer.kernel_flags = flags
    GraphPlan.clear_cache()
    with torch.no_grad():
        out = layer(*[None if t is None else t.to(DEV) for t in graph])
    torch.cuda.synchronize()
    return out.cpu(), layer.att.cpu()


def _one_tile(E):
    """E edges of one relation into the first 256-target tile"""
    N, d, H, T, R = 300, 256, 8, 2, 1
    x, nt, ei, et, _ = synthetic_typed_graph(N, max(E, 2), d, T, R, seed=100 + E)
    ei, et = ei[:, :E].clone(), torch.zeros(E, dtype=et.dtype)
    ei[1] %= 256
    return (d, H, T, R), (x, nt, ei.contiguous(), et, None)


def _mixed():
    N, E, d, H, T, R = 600, 5000, 256, 8, 3, 3
    x, nt, ei, et, _ = synthetic_typed_graph(N, E, d, T, R, seed=E + 7)
    et = et.clone()
    et[::41] = R                      # unclaimed items between claimed ones
    return (d, H, T, R), (x, nt, ei, et, None)


def _long_items(d, H):
    """270 000 edges: the default route's own 64-edge items, many batches per item"""
    N, E, T, R = 400, 270000, 2, 3
    x, nt, ei, et, _ = synthetic_typed_graph(N, E, d, T, R, seed=E + 7)
    et = et.clone()
    et[::41] = R
    return (d, H, T, R), (x, nt, ei, et, None)


def _one_source_one_target():
    """every edge of an item from ONE source row, and every edge of another to ONE target: identical lines inside a piece"""
    N, E, d, H, T, R = 600, 4000, 256, 8, 2, 2
    x, nt, ei, et, _ = synthetic_typed_graph(N, E, d, T, R, seed=31)
    ei, et = ei.clone(), et.clone()
    ei[0, :200], ei[1, :200], et[:200] = 17, ei[1, :200] % 256, 0              # one source, tile 0
    ei[0, 200:400], ei[1, 200:400], et[200:400] = ei[0, 200:400], 300, 1      # one target
    return (d, H, T, R), (x, nt, ei, et, None)


def _last_rows():
    """sources are the last rows of the table: no piece reads past it (a read behind the table returns zeros, not the row)"""
    N, E, d, H, T, R = 520, 3000, 256, 8, 2, 2
    x, nt, ei, et, _ = synthetic_typed_graph(N, E, d, T, R, seed=77)
    ei = ei.clone()
    ei[0] = N - 1 - (ei[0] % 9)
    return (d, H, T, R), (x, nt, ei, et, None)


GRAPHS = {
    **{"tile-e%d" % E: (lambda E=E: _one_tile(E)) for E in (1, 7, 8, 9, 31, 32, 33, 65)},
    "mixed-n600-e5000": _mixed,
    "long-d64-h2": lambda: _long_items(64, 2),
    "long-d128-h4": lambda: _long_items(128, 4),
    "one-source-one-target": _one_source_one_target,
    "last-rows": _last_rows,
}
WITH_REFERENCE = tuple("tile-e%d" % E for E in (1, 7, 8, 9, 31, 32, 33, 65)) + ("mixed-n600-e5000", "long-d64-h2")
_shared = {}


def _graph(name):
    """graph, weights and (for the graphs of WITH_REFERENCE) the fp64 reference: made once, shared by the precisions, never modified"""
    if name not in _shared:
        (d, H, T, R), graph = GRAPHS[name]()
        sd = O.make_state_dict(d, d, T, R, H, True, False, seed=len(name) + d)
        ref = None
        if name in WITH_REFERENCE:
            ref = O.forward_closed_form(sd, T, R, H, *graph, use_norm=True, use_RTE=False, dtype=torch.float64, return_att=True)
        _shared[name] = ((d, H, T, R), graph, sd, ref)
    return _shared[name]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_lds_gather_is_bit_identical_to_the_lane_gather(name, precision):
    (d, H, T, R), graph, sd, ref = _graph(name)
    layer = _layer(sd, d, T, R, H, precision)
    out, att = _run(layer, graph, KSIDE)
    out_l, att_l = _run(layer, graph, LANE)
    n_out, n_att = int((out != out_l).sum()), int((att != att_l).sum())
    print("kside gather %s %s: %d of %d outputs and %d of %d attention weights differ from the lane gather"
          % (name, precision, n_out, out.numel(), n_att, att.numel()))
    assert torch.isfinite(out).all() and torch.isfinite(att).all()
    assert torch.equal(att, att_l)
    assert torch.equal(out, out_l)
    if ref is not None:
        err, err_att = (out.double() - ref[0]).abs().max().item(), (att.double() - ref[1]).abs().max().item()
        print("   against the fp64 closed form: max|out| err %.2e, att err %.2e" % (err, err_att))
        assert err < PREC_TOL[precision]
        assert err_att < ATT_TOL[precision]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_runs_of_the_lds_gather_are_bit_identical(precision):
    (d, H, T, R), graph, sd, _ = _graph("long-d64-h2")
    layer = _layer(sd, d, T, R, H, precision)
    out, att = _run(layer, graph, KSIDE)
    out2, att2 = _run(layer, graph, KSIDE)
    assert torch.equal(out, out2) and torch.equal(att, att2)


@pytest.mark.parametrize("flags", [KSIDE, LANE], ids=["lds", "lane"])
def test_stage5_item_ranges_are_bit_identical_to_the_one_call_layer(flags):
    """the range form of the kernel (hgt_conv_forward stage 5), two item ranges: the one-call layer bit for bit, in either form"""
    N, E, d, H, T, R = 17000, 120000, 256, 8, 3, 4      # (from 16384 targets on the one-call layer takes the fused aggregation of stage 5)
    sd = O.make_state_dict(d, d, T, R, H, True, False, seed=61)
    x, nt, ei, et, _ = synthetic_typed_graph(N, E, d, T, R, seed=62)
    et = et.clone()
    et[::41] = R
    layer = HGTConv(d, d, T, R, H, 0.2, True, False, keep_att=False, precision="bf16x3").eval()
    layer.load_state_dict(sd)
    layer = layer.to(DEV)
    layer.kernel_flags = flags
    xd, ntd, eid, etd = (t.to(DEV) for t in (x, nt, ei, et))
    GraphPlan.clear_cache()
    plan = GraphPlan(ntd, eid, etd, None, T, R, n_q_rows=N)
    ws = torch.empty(layer.workspace_bytes(N, E), dtype=torch.uint8, device=DEV)
    args, kw = (xd, ntd, eid, etd, None), dict(plan=plan, n_q_rows=N, workspace=ws)
    with torch.no_grad():
        ref = layer(*args, **kw).clone()
        tab, tile = plan.tile_items()
        out = torch.full((N, d), float("nan"), device=DEV)
        layer(*args, stage=1, **kw)
        bounds = [0, 29 * tile, N]
        for b in (1, 0):
            q0, q1 = bounds[b], bounds[b + 1]
            layer(*args, stage=5, block=(q0, q1, int(tab[q0 // tile]), int(tab[(q1 + tile - 1) // tile])), out=out, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    if flags == LANE:      # ... and the two forms agree on the one-call layer
        layer.kernel_flags = KSIDE
        with torch.no_grad():
            assert torch.equal(layer(*args, **kw), ref)
