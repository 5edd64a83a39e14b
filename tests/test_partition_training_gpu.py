"""GPU tests of training on a destination partition: hgt_scatter_add_rows (the kernel that adds returned halo gradients into the
owners' rows), the rectangular training step (targets [0, NQ), source-only rows [NQ, N)) against the fp64 oracle, and the
partitioned step -- three ranks played one after another on one GPU, three processes on one GPU, and the example script.

The oracle of a rectangular step is oracle.hgt_oracle.backward_reference on the same graph with the source-only rows as ordinary
nodes without in-edges and a zero grad_out on them; bounds: test_backward_gpu._grads_close (RTOL, ENTRY_RTOL, ENTRY_ATOL)."""
import os
import re
import socket
import subprocess
import sys

import pytest
import torch

import test_backward_gpu as BG
import test_hgt_gpu as HG
from oracle import hgt_oracle as O
from pyhgt_amd import DenseHGTConv, GraphPlan, HGTConv, _lib, set_deterministic
from pyhgt_amd.autograd import spmm_takes_items, training_supported
from pyhgt_amd.synth import synthetic_typed_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# == the kernel =================================================================================================================
N_DST, N_LISTED, N_SRC = 400, 301, 700
MULT = [7] * 50 + [3] * 80 + [1] * 110 + [0] * 61      # 301 listed rows, 700 source rows in all


def _scatter_problem(d, seed=0):
    g = torch.Generator().manual_seed(seed)
    mult = torch.tensor(MULT)[torch.randperm(N_LISTED, generator=g)]
    assert mult.numel() == N_LISTED and int(mult.sum()) == N_SRC
    rows = torch.sort(torch.randperm(N_DST, generator=g)[:N_LISTED]).values.to(torch.int32)
    ptr = torch.zeros(N_LISTED + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(mult, 0)
    pos = torch.randperm(N_SRC, generator=g).to(torch.int32)       # every source row belongs to one destination row
    src = torch.randn(N_SRC, d, generator=g)
    dst = torch.randn(N_DST, d, generator=g)
    return rows, ptr, pos, src, dst, mult


def _scatter_reference(rows, ptr, pos, src, dst, mult):
    """fp32 on the CPU, in the documented order: dst, then the listed source rows one after the other."""
    out = dst.clone()
    acc = out[rows.long()]
    for k in range(int(mult.max())):
        m = mult > k
        acc[m] = acc[m] + src[pos[(ptr[:-1][m] + k).long()].long()]
    out[rows.long()] = acc
    return out


def _padded(t, ld, shift=0):
    """t [n, d] as a device view with leading dimension ld whose first element sits `shift` floats behind a 256-byte boundary."""
    n, d = t.shape
    buf = torch.full((n * ld + shift + 8,), float("nan"), device=DEV)
    view = buf[shift:shift + n * ld].view(n, ld)[:, :d]
    view.copy_(t.to(DEV))
    return buf, view


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "misaligned_base"])
@pytest.mark.parametrize("d", [30, 64, 200, 1024])
def test_scatter_add_rows_is_bit_equal_to_the_ordered_cpu_sum(d, shift):
    lib = _lib.load()
    rows, ptr, pos, src, dst, mult = _scatter_problem(d, seed=d)
    ref = _scatter_reference(rows, ptr, pos, src, dst, mult)
    ld_src, ld_dst = d + 8, d + 4                      # both larger than d; multiples of 4 where d is, so that d = 64, 200, 1024 with
    rd, pd, qd = rows.to(DEV), ptr.to(DEV), pos.to(DEV)      # an aligned base take the 16-byte path, and every d with shift = 1 the scalar one
    results = []
    for _ in range(2):
        sbuf, sv = _padded(src, ld_src, shift)
        dbuf, dv = _padded(dst, ld_dst, shift)
        assert (sv.data_ptr() % 16 == 0) == (shift == 0) and sv.stride(0) == ld_src and dv.stride(0) == ld_dst
        assert lib.hgt_scatter_add_rows(sv.data_ptr(), ld_src, rd.data_ptr(), pd.data_ptr(), qd.data_ptr(), N_LISTED, d, dv.data_ptr(),
                                        ld_dst, _stream()) == 0
        torch.cuda.synchronize()
        results.append(dv.cpu())
        # the padding columns and the guard floats around the view were not written
        pad = dbuf[shift:shift + N_DST * ld_dst].view(N_DST, ld_dst)[:, d:]
        assert bool(torch.isnan(pad).all()) and bool(torch.isnan(dbuf[:shift]).all()) and bool(torch.isnan(dbuf[shift + N_DST * ld_dst:]).all())
    assert torch.equal(results[0], ref), "%d rows differ from the ordered fp32 sum" % int((results[0] != ref).any(1).sum())
    assert torch.equal(results[0], results[1])
    listed = torch.zeros(N_DST, dtype=torch.bool)
    listed[rows.long()[mult > 0]] = True
    assert torch.equal(results[0][~listed], dst[~listed])          # rows not listed (or listed with nothing to add) are untouched
    assert bool((results[0][listed] != dst[listed]).any(1).all())


def test_scatter_add_rows_argument_contract():
    lib = _lib.load()
    d = 64
    rows, ptr, pos, src, dst, mult = _scatter_problem(d)
    rd, pd, qd, sd_, dd = (t.to(DEV) for t in (rows, ptr, pos, src, dst))
    before = dd.clone()
    args = lambda **kw: [kw.get("src", sd_.data_ptr()), kw.get("ld_src", d), kw.get("rows", rd.data_ptr()), kw.get("ptr", pd.data_ptr()),
                         kw.get("pos", qd.data_ptr()), kw.get("n", N_LISTED), kw.get("d", d), kw.get("dst", dd.data_ptr()),
                         kw.get("ld_dst", d), _stream()]
    assert lib.hgt_scatter_add_rows(*args(n=0)) == 0                       # nothing to do: no launch ...
    assert lib.hgt_scatter_add_rows(*args(n=0, src=None, dst=None)) == 0
    torch.cuda.synchronize()
    assert torch.equal(dd, before)                                         # ... and the destination keeps its bits
    for bad in (dict(src=None), dict(rows=None), dict(ptr=None), dict(pos=None), dict(dst=None), dict(n=-1), dict(d=0), dict(d=-3),
                dict(ld_src=d - 1), dict(ld_dst=d - 1)):
        assert lib.hgt_scatter_add_rows(*args(**bad)) == -1, bad           # HGT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert torch.equal(dd, before)


# == one layer, rectangular, against the oracle ====================================================================================
def _rect_graph(name):
    """(T, R, H, d, N, NQ, use_norm, use_RTE, x, nt, ei, et, tm): every edge's target is below NQ."""
    if name == "c1_rect":              # NQ is no multiple of 64
        T, R, H, d, N, NQ, E, norm, rte, gk = 3, 4, 4, 64, 2000, 1300, 10000, True, True, {}
    elif name == "dk50_unsorted":      # d_k = 50 (padded heads), unsorted types, unknown types among targets and halo rows, unclaimed edges
        T, R, H, d, N, NQ, E, norm, rte, gk = 2, 3, 4, 200, 1500, 700, 9000, True, True, dict(sorted_types=False)
    elif name == "hubs":               # a hub target and a hub of the transposed plan beyond NQ
        T, R, H, d, N, NQ, E, norm, rte, gk = 3, 5, 2, 32, 3000, 1800, 30000, True, True, dict(sorted_types=False)
    elif name == "sub_tile_70k":       # from 65 536 nodes the gather passes take the sub-tile hgt_edge_spmm
        T, R, H, d, N, NQ, E, norm, rte, gk = 3, 4, 2, 32, 70000, 40000, 300000, True, False, dict(sorted_types=False)
    else:
        raise KeyError(name)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=len(name) + N, **gk)
    nt, et, ei = nt.clone(), et.clone(), ei.clone().contiguous()
    ei[1] %= NQ
    if name == "dk50_unsorted":
        nt[::13] = T + 1
        assert bool((nt[:NQ] > T).any()) and bool((nt[NQ:] > T).any())
        et[::7] = R
    if name == "hubs":
        ei[1, :4000] = 17                   # a target with 4 000 in-edges
        ei[0, 4000:7000] = NQ + 23          # a halo row with 3 000 out-edges
    if name == "sub_tile_70k":
        dp = _lib.layout_for(d, H).d_pad
        assert not any(spmm_takes_items(N, E, R, ld, col) for ld, col in ((dp, 0), (3 * dp, 0), (3 * dp, dp), (3 * dp, 2 * dp)))
    return T, R, H, d, N, NQ, norm, rte, x, nt, ei, et, tm


_REF_CACHE = {}


def _rect_reference(name, dense=False, drop_masks=None):
    """The graph, grad_out and the fp64 oracle gradients of a case: computed once, shared by the precisions, never modified."""
    key = (name, dense)
    if key not in _REF_CACHE or drop_masks is not None:
        T, R, H, d, N, NQ, norm, rte, x, nt, ei, et, tm = graph = _rect_graph(name)
        sd = O.make_state_dict(d, d, T, R, H, norm, rte, seed=61, dense=dense)
        gout = torch.zeros(N, d)
        gout[:NQ] = torch.randn(NQ, d, generator=torch.Generator().manual_seed(62))      # zero on the halo rows
        ref = O.backward_reference(sd, T, R, H, x, nt, ei, et, tm if rte else None, gout, use_norm=norm, use_RTE=rte, dense=dense,
                                   drop_masks=drop_masks)
        fwd = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm if rte else None, use_norm=norm, use_RTE=rte, dense=dense,
                                    drop_masks=drop_masks)
        if drop_masks is not None:
            return graph, sd, gout, ref, fwd
        _REF_CACHE[key] = (graph, sd, gout, ref, fwd)
    return _REF_CACHE[key]


def _make_layer(graph, sd, precision, dense=False, p=0.2):
    T, R, H, d, N, NQ, norm, rte = graph[:8]
    layer = (DenseHGTConv if dense else HGTConv)(d, d, T, R, H, p, norm, rte, precision=precision)
    layer.load_state_dict(sd)
    return layer.to(DEV)


def _run_rect(layer, graph, gout, n_q_rows="NQ"):
    T, R, H, d, N, NQ, norm, rte, x, nt, ei, et, tm = graph
    xd = x.to(DEV).requires_grad_(True)
    GraphPlan.clear_cache()
    layer.zero_grad()
    nq = NQ if n_q_rows == "NQ" else n_q_rows
    out = layer(xd, nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV) if rte else None, n_q_rows=nq)
    out.backward(gout[:out.size(0)].to(DEV))
    torch.cuda.synchronize()
    return out.detach(), xd.grad


def _compare(label, layer, out, xgrad, graph, ref, fwd):
    N, NQ, d = graph[4], graph[5], graph[3]
    assert out.shape == (NQ, d) and xgrad.shape == (N, d)
    assert (out.cpu().double() - fwd[:NQ]).abs().max().item() < 1e-4
    worst = BG._grads_close("x", xgrad, ref["x"])              # all N rows: skip + Q + K + V on the targets, K + V on the halo rows
    assert bool((ref["x"][NQ:] != 0).any())
    for k, p in layer.named_parameters():
        if k == "emb.emb.weight" and p.grad is None:
            continue
        assert p.grad is not None, k
        worst = max(worst, BG._grads_close(k, p.grad, ref[k]))
    print("rectangular %s: worst relative gradient error %.2e" % (label, worst))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["c1_rect", "dk50_unsorted", "hubs", "sub_tile_70k"])
def test_rectangular_hgtconv_step_matches_the_oracle(name, precision):
    graph, sd, gout, ref, fwd = _rect_reference(name)
    layer = _make_layer(graph, sd, precision).eval()
    out, xgrad = _run_rect(layer, graph, gout)
    _compare("%s / %s" % (name, precision), layer, out, xgrad, graph, ref, fwd)


def test_rectangular_dense_hgtconv_step_matches_the_oracle():
    graph, sd, gout, ref, fwd = _rect_reference("c1_rect", dense=True)
    layer = _make_layer(graph, sd, "bf16x3", dense=True).eval()
    out, xgrad = _run_rect(layer, graph, gout)
    _compare("dense c1_rect / bf16x3", layer, out, xgrad, graph, ref, fwd)


# == smaller checks ================================================================================================================
@pytest.mark.parametrize("conv", ["hgt", "dense"])
def test_rectangular_dropout_masks_cover_the_targets_and_gradients_match(conv, monkeypatch):
    dense = conv == "dense"
    graph = _rect_graph("c1_rect")
    T, R, H, d, N, NQ = graph[:6]
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=61, dense=dense)
    p = 0.3
    layer = _make_layer(graph, sd, "bf16x3", dense=dense, p=p).train()
    drawn, real_bernoulli = [], torch.bernoulli

    def recording_bernoulli(*a, **k):
        out = real_bernoulli(*a, **k)
        drawn.append(out.clone())
        return out

    monkeypatch.setattr(torch, "bernoulli", recording_bernoulli)
    gout = torch.zeros(N, d)
    gout[:NQ] = torch.randn(NQ, d, generator=torch.Generator().manual_seed(62))
    out, xgrad = _run_rect(layer, graph, gout)
    monkeypatch.undo()
    assert len(drawn) == (2 if dense else 1) and all(m.shape == (NQ, d) for m in drawn)
    masks = []
    for m in drawn:      # the oracle runs on all N nodes: the halo rows (zero grad_out, nobody's source of an update) keep everything
        full = torch.ones(N, d)
        full[:NQ] = (m / (1.0 - p)).cpu()
        masks.append(full)
    dm = (masks[0], masks[1] if dense else None)
    _, _, _, ref, fwd = _rect_reference("c1_rect", dense=dense, drop_masks=dm)
    _compare("dropout %s" % conv, layer, out, xgrad, graph, ref, fwd)


def _all_grads(layer, out, xgrad):
    return [out.clone(), xgrad.clone()] + [p.grad.clone() for _, p in sorted(layer.named_parameters()) if p.grad is not None]


def test_square_step_with_explicit_n_q_rows_gives_the_bits_of_the_plain_call():
    graph, sd, gout, _, _ = _rect_reference("c1_rect")
    N = graph[4]
    square = graph[:5] + (N,) + graph[6:]
    layer = set_deterministic(_make_layer(graph, sd, "bf16x3").eval())
    a = _all_grads(layer, *_run_rect(layer, square, torch.ones(N, graph[3]) * gout.abs().max(), n_q_rows=N))
    b = _all_grads(layer, *_run_rect(layer, square, torch.ones(N, graph[3]) * gout.abs().max(), n_q_rows=None))
    assert len(a) == len(b) > 10 and a[0].shape == (N, graph[3])
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("name", ["c1_rect", "hubs"])
def test_deterministic_rectangular_step_repeats_bit_for_bit(name):
    graph, sd, gout, _, _ = _rect_reference(name)
    layer = set_deterministic(_make_layer(graph, sd, "bf16x3", p=0.2).train())
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        runs.append(_all_grads(layer, *_run_rect(layer, graph, gout)))
    assert len(runs[0]) == len(runs[1]) > 10
    assert all(torch.equal(u, v) for u, v in zip(*runs))


def test_staged_calls_under_grad_still_raise_and_wide_heads_keep_their_reason():
    graph, sd, gout, _, _ = _rect_reference("c1_rect")
    T, R, H, d, N, NQ, norm, rte, x, nt, ei, et, tm = graph
    layer = _make_layer(graph, sd, "bf16x3").eval()
    args = (x.to(DEV).requires_grad_(True), nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV))
    ws = torch.empty(layer.workspace_bytes(N, ei.size(1)), dtype=torch.uint8, device=DEV)
    for stage in (1, 2, 3, 4, 5):
        with pytest.raises(RuntimeError, match="no_grad"):
            layer(*args, n_q_rows=NQ, stage=stage, workspace=ws)
    # a head wider than 256 padded columns: training_supported's reason, before anything runs
    ok, reason = training_supported(512, 1)
    assert not ok and "at most 256" in reason
    wide = HGTConv(512, 512, 2, 2, 1, use_RTE=False).to(DEV)
    n, nq = 96, 50
    xw = torch.randn(n, 512, device=DEV, requires_grad=True)
    ntw = torch.zeros(n, dtype=torch.long, device=DEV)
    eiw = torch.stack([torch.arange(n, device=DEV), torch.arange(n, device=DEV) % nq])
    etw = torch.zeros(n, dtype=torch.long, device=DEV)
    with pytest.raises(NotImplementedError, match="at most 256"):
        wide(xw, ntw, eiw, etw, n_q_rows=nq)


def test_a_step_without_targets_and_a_mismatched_n_q_rows_are_rejected():
    graph, sd, gout, _, _ = _rect_reference("c1_rect")
    T, R, H, d, N, NQ, norm, rte, x, nt, ei, et, tm = graph
    layer = _make_layer(graph, sd, "bf16x3").eval()
    xd = x.to(DEV).requires_grad_(True)
    none = torch.zeros(2, 0, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="at least one target"):
        layer(xd, nt.to(DEV), none, none[0], none[0], n_q_rows=0)
    plan = GraphPlan(nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV), T, R, n_q_rows=NQ)
    with pytest.raises(ValueError, match="plan was built with n_q_rows=%d" % NQ):
        layer(xd, nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV), plan=plan, n_q_rows=NQ + 1)


def test_training_is_refused_on_every_rank_when_a_rank_owns_no_targets():
    """Rank 1 of 2 owns nothing.  Rank 0 -- which HAS targets, and whose input does not require grad -- refuses the step from the
    shared offsets, before the exchange: no rank is left waiting in a collective the empty rank's backward would never enter.
    Inference on the same partition still runs."""
    from pyhgt_amd.dist import HaloPlan, PartitionedGraph
    T, R, H, d, N, E = 3, 4, 4, 64, 600, 4000
    x, nt, ei, et, tm = (t.to(DEV) for t in synthetic_typed_graph(N, E, d, T, R, seed=5, sorted_types=False))
    offsets = [0, N, N]
    hp = HaloPlan(nt, ei[0].contiguous(), offsets, 0, 2, emulate={"node_type_global": nt})
    assert hp.n_halo == 0 and hp.n_own == N
    pg = PartitionedGraph(None, None, ei[1].contiguous(), et, tm, T, R, 0, 0, 2, node_offsets=offsets, halo=hp, mode="pipelined", n_chunks=1)
    layer = HGTConv(d, d, T, R, H, precision="bf16x3").to(DEV).train()
    assert not x.requires_grad
    with pytest.raises(RuntimeError, match=r"rank\(s\) \[1\] own none"):
        pg.forward(layer, x)
    with torch.no_grad():
        assert pg.forward(layer.eval(), x).shape == (N, d)


# == three ranks, one after another, on one GPU ====================================================================================
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


HALO_N, HALO_E, HALO_D, HALO_T, HALO_R, HALO_H = 900, 9000, 64, 3, 4, 4
HALO_OFFSETS = [0, 250, 610, 900]


def test_three_ranks_one_after_another_stitch_to_the_global_gradients(tmp_path):
    """Every rank's rectangular step on its [own ; halo] rows; the test plays the reverse all-to-all (slices of the peers' d_local
    halo rows by recv_chunk_splits, assembled in the owner's send-list order) and hands the buffer to the library's reduce step:
    HaloPlan.return_index + hgt_scatter_add_rows."""
    import torch.multiprocessing as mp
    N, E, d, T, R, H, world, n_chunks, offsets = HALO_N, HALO_E, HALO_D, HALO_T, HALO_R, HALO_H, 3, 3, HALO_OFFSETS
    mp.spawn(HG._halo_worker, args=(world, _free_port(), N, E, d, T, R, offsets, n_chunks, str(tmp_path)), nprocs=world, join=True)
    x, nt, ei, et, tm = HG._halo_graph(N, E, d, T, R, offsets, False)
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=92)
    gout = torch.randn(N, d, generator=torch.Generator().manual_seed(93))
    ref = O.backward_reference(sd, T, R, H, x, nt, ei, et, tm, gout)
    layer = HGTConv(d, d, T, R, H, 0.2, True, True, precision="bf16x3").eval()
    layer.load_state_dict(sd)
    layer = layer.to(DEV)
    lib = _lib.load()
    plans, d_locals, param_sum = [], [], {}
    for rank in range(world):
        lo, hi = offsets[rank], offsets[rank + 1]
        mine = (ei[1] >= lo) & (ei[1] < hi)
        hp = torch.load(os.path.join(str(tmp_path), "halo%d.pt" % rank), weights_only=False).to(DEV)
        gid = torch.cat([torch.arange(lo, hi), hp.need[hp.halo_order].cpu()])
        x_local = x[gid].to(DEV).requires_grad_(True)                          # a leaf filled from the global table
        ei_local = torch.stack([hp.src_local, (ei[1][mine] - lo).to(DEV)])
        GraphPlan.clear_cache()
        layer.zero_grad()
        out = layer(x_local, hp.node_type_local, ei_local, et[mine].to(DEV), tm[mine].to(DEV), n_q_rows=hp.n_own)
        assert out.shape == (hi - lo, d)
        out.backward(gout[lo:hi].to(DEV))
        plans.append(hp)
        d_locals.append(x_local.grad.clone())
        for k, p in layer.named_parameters():
            if p.grad is not None:
                param_sum[k] = param_sum.get(k, 0) + p.grad.double().cpu()
    dx = torch.empty(N, d)
    for rank in range(world):
        hp, lo, hi = plans[rank], offsets[rank], offsets[rank + 1]
        recv = torch.full((hp.send_rows.numel(), d), float("nan"), device=DEV)
        for c in range(n_chunks):                                             # chunk c: from every peer q its halo rows of (chunk c, owner = rank)
            at = hp.send_chunk_off[c]
            for q in range(world):
                n = hp.send_chunk_splits[c][q]
                hq = plans[q]
                assert hq.recv_chunk_splits[c][rank] == n
                a = hq.n_own + hq.recv_chunk_off[c] + sum(hq.recv_chunk_splits[c][:rank])
                recv[at:at + n] = d_locals[q][a:a + n]
                at += n
            assert at == hp.send_chunk_off[c + 1]
        d_own = d_locals[rank][:hp.n_own].clone()
        rows, ptr, pos = hp.return_index(DEV)
        assert rows.numel() > 0 and int(ptr[-1]) == hp.send_rows.numel()
        assert lib.hgt_scatter_add_rows(recv.data_ptr(), d, rows.data_ptr(), ptr.data_ptr(), pos.data_ptr(), rows.numel(), d,
                                        d_own.data_ptr(), d, _stream()) == 0
        torch.cuda.synchronize()
        dx[lo:hi] = d_own.cpu()
    worst = BG._grads_close("x", dx, ref["x"])
    for k, g in param_sum.items():
        worst = max(worst, BG._grads_close(k, g, ref[k]))
    assert set(param_sum) >= {k for k in ref if k != "x" and k != "emb.emb.weight"}
    print("three ranks in turn: worst relative gradient error %.2e" % worst)


# == three processes on one GPU ====================================================================================================
def _train_worker(rank, world, port, tmpdir):
    import datetime
    import torch.distributed as dist
    from pyhgt_amd.dist import PartitionedGraph, all_reduce_grads, partition
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        N, E, d, T, R, H, offsets = HALO_N, HALO_E, HALO_D, HALO_T, HALO_R, HALO_H, HALO_OFFSETS
        torch.cuda.set_device(0)
        x, nt, ei, et, tm = HG._halo_graph(N, E, d, T, R, offsets, False)
        part = partition(nt, ei, et, tm, world, rank, node_offsets=offsets)
        lo, hi = offsets[rank], offsets[rank + 1]
        pg = PartitionedGraph(part["node_type_own"].to(DEV), part["src_global"].to(DEV), part["dst_local"].to(DEV),
                              part["edge_type"].to(DEV), part["edge_time"].to(DEV), T, R, 0, rank, world, node_offsets=offsets,
                              n_chunks=3, mode="blocked")
        layers = torch.nn.ModuleList()
        for i in range(2):
            layer = HGTConv(d, d, T, R, H, 0.2, True, True, precision="bf16x3")
            layer.load_state_dict(O.make_state_dict(d, d, T, R, H, True, True, seed=92 + i))
            layers.append(layer)
        layers = layers.to(DEV).eval()
        gout = torch.randn(N, d, generator=torch.Generator().manual_seed(93))
        x_own = x[lo:hi].to(DEV).requires_grad_(True)
        h = x_own
        for layer in layers:
            h = pg.forward(layer, h)
        assert h.shape == (hi - lo, d) and h.requires_grad
        h.backward(gout[lo:hi].to(DEV))
        all_reduce_grads(layers)
        torch.cuda.synchronize()
        torch.save(dict(x_grad=x_own.grad.cpu(), out=h.detach().cpu(), params={k: p.grad.cpu() for k, p in layers.named_parameters()
                                                                               if p.grad is not None}),
                   os.path.join(tmpdir, "train%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_three_processes_on_one_gpu_train_two_chained_layers(tmp_path):
    import torch.multiprocessing as mp
    N, E, d, T, R, H, world, offsets = HALO_N, HALO_E, HALO_D, HALO_T, HALO_R, HALO_H, 3, HALO_OFFSETS
    mp.spawn(_train_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(str(tmp_path), "train%d.pt" % r)) for r in range(world)]
    # fp64 autograd through two closed-form layers on the whole graph
    x, nt, ei, et, tm = HG._halo_graph(N, E, d, T, R, offsets, False)
    gout = torch.randn(N, d, generator=torch.Generator().manual_seed(93))
    xg = x.double().requires_grad_(True)
    leaves, h = [], xg
    for i in range(2):
        sd = O.make_state_dict(d, d, T, R, H, True, True, seed=92 + i)
        leaf = {k: v.double().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
        leaves.append(leaf)
        h = O.forward_closed_form(leaf, T, R, H, h, nt, ei, et, tm, dtype=torch.float64)
    names = [(i, k) for i in range(2) for k in leaves[i]]
    grads = torch.autograd.grad((h * gout.double()).sum(), [xg] + [leaves[i][k] for i, k in names], allow_unused=True)
    ref = {"%d.%s" % ik: g for ik, g in zip(names, grads[1:]) if g is not None}
    out = torch.cat([g["out"] for g in got])
    # (a layer's output is within 1e-4 of fp64, the bound of every forward test here; the second layer's LayerNorm'd rows are O(1)
    #  like the first's, and it sees an input that is off by as much: twice the bound)
    assert (out.double() - h.detach()).abs().max().item() < 2e-4
    worst = BG._grads_close("x", torch.cat([g["x_grad"] for g in got]), grads[0])
    for k, g in got[0]["params"].items():
        if k.endswith("emb.emb.weight"):
            continue
        worst = max(worst, BG._grads_close(k, g, ref[k]))
    assert len(got[0]["params"]) >= 2 * 10
    for r in range(1, world):      # after the all-reduce every rank holds the same parameter gradients
        assert got[r]["params"].keys() == got[0]["params"].keys()
        assert all(torch.equal(got[r]["params"][k], got[0]["params"][k]) for k in got[0]["params"])
    print("three processes, two layers: worst relative gradient error %.2e" % worst)


# == the example ===================================================================================================================
def test_partitioned_training_example_reduces_the_loss():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc-per-node", "2",
           os.path.join(ROOT, "examples", "train_partitioned.py"), "--backend", "gloo", "--device-index", "0", "--steps", "12",
           "--nodes", "3000", "--edges", "30000"]
    res = subprocess.run(cmd, cwd=ROOT, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    for rank in range(2):
        losses = [float(v) for v in re.findall(r"rank %d step +\d+ loss ([0-9.eE+-]+)" % rank, res.stdout)]      # (no line anchor: the ranks share one stdout)
        assert len(losses) == 12, res.stdout[-3000:]
        assert losses[-1] < losses[0], (rank, losses)
