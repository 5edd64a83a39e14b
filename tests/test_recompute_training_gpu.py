"""GPU tests of the memory-lean training mode (recompute=True): the counter-based dropout kernels against the numpy restatement of
tests/test_recompute_training.py (exact), hgt_dropout_apply against hgt_mul_inplace (bit-equal), the promise the mode rests on
(a step run twice gives the same bits), whole layers in both modes (bit-equal without dropout, against the fp64 oracle with the
masks of the layer's seed), the memory a forward keeps, and a short training loop."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_backward_gpu as BG
import test_partition_training_gpu as PT
import test_recompute_training as RT
from oracle import hgt_oracle as O
import pyhgt_amd
from pyhgt_amd import HGTConv, DenseHGTConv, GNN, Classifier, GraphPlan, _lib
from pyhgt_amd.autograd import _Step, spmm_takes_items
from pyhgt_amd.synth import synthetic_typed_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _mask(n, seed, offset, keep):
    m = torch.full((n + 2,), -7.0, device=DEV)      # the array starts 4 bytes past an aligned address half of the time (n odd / even)
    assert _lib.load().hgt_dropout_mask(m.data_ptr() + 4, n, seed, offset, keep, _st()) == 0
    torch.cuda.synchronize()
    assert m[0].item() == -7.0 and m[n + 1].item() == -7.0, "hgt_dropout_mask wrote outside [0, n)"
    return m[1:n + 1]


# -- 1. the mask kernel is the restatement -------------------------------------------------------------------------------------
SEEDS = [0, 2 ** 63 + 12345]
OFFSETS = [0, 2 ** 32 - 2, 2 ** 40]          # 2^32 - 2: the third group carries into counter word 1
SIZES = [1, 3, 4, 5, 255, 256, 257, 65537]


@pytest.mark.parametrize("keep", [0.8, 0.5, 1.0, 0.0])
def test_dropout_mask_equals_the_restatement(keep):
    lib = _lib.load()
    for seed in SEEDS:
        for offset in OFFSETS:
            ref_all = RT.dropout_mask_reference(max(SIZES), seed, offset, keep)         # a prefix of it is the mask of a smaller n
            for n in SIZES:
                for shift in (0, 1):                                                   # 16-byte aligned, and one float past it
                    buf = torch.full((n + 8,), -7.0, device=DEV)
                    assert lib.hgt_dropout_mask(buf.data_ptr() + 4 * (4 + shift), n, seed, offset, keep, _st()) == 0
                    got = buf.cpu().numpy()
                    lo = 4 + shift
                    assert np.array_equal(got[lo:lo + n].view(np.uint32), ref_all[:n].view(np.uint32)), (n, seed, offset, keep, shift)
                    assert (got[:lo] == -7.0).all() and (got[lo + n:] == -7.0).all(), "wrote outside [0, n)"
    if 0.0 < keep < 1.0:
        assert set(np.unique(ref_all).tolist()) == {0.0, float(np.float32(1) / np.float32(keep))}


# -- 2. apply == mul_inplace by that mask --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257, 65537])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one_float_off"])
def test_dropout_apply_is_bit_equal_to_mul_inplace(n, shift):
    lib = _lib.load()
    seed, offset, keep = 2 ** 63 + 12345, 2 ** 32 - 2, 0.8
    g = torch.Generator(device=DEV).manual_seed(n)
    data = torch.randn(n, generator=g, device=DEV)
    mask = torch.from_numpy(RT.dropout_mask_reference(n, seed, offset, keep)).to(DEV)
    a, b = (torch.full((n + 8,), -7.0, device=DEV) for _ in range(2))
    lo = 4 + shift
    a[lo:lo + n] = data
    b[lo:lo + n] = data
    assert lib.hgt_dropout_apply(a.data_ptr() + 4 * lo, n, seed, offset, keep, _st()) == 0
    assert lib.hgt_mul_inplace(b.data_ptr() + 4 * lo, mask.data_ptr(), n, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))                       # the sentinels on both sides included
    assert bool((a[:lo] == -7.0).all() and (a[lo + n:] == -7.0).all())
    # keep >= 1 leaves the array as it is, keep <= 0 zeroes it
    c = data.clone()
    assert lib.hgt_dropout_apply(c.data_ptr(), n, seed, offset, 1.0, _st()) == 0
    assert torch.equal(_bits(c), _bits(data))
    assert lib.hgt_dropout_apply(c.data_ptr(), n, seed, offset, 0.0, _st()) == 0
    assert bool((c == 0).all())


def test_dropout_kernels_over_several_passes_of_the_grid():
    """n = 2^24 + 5: more groups than any grid has lanes (the kernel strides), a tail of one element, and enough elements for the
    kept fraction: within 5 sigma = 5 sqrt(0.8 * 0.2 / n) = 4.9e-4 of 0.8."""
    lib = _lib.load()
    n, seed, offset, keep = 2 ** 24 + 5, 2 ** 63 + 12345, 2 ** 40, 0.8
    ref = RT.dropout_mask_reference(n, seed, offset, keep)
    m = _mask(n, seed, offset, keep)                              # one float past an aligned address: the element-wise path
    assert np.array_equal(m.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    mask = torch.full((n + 4,), -7.0, device=DEV)
    assert lib.hgt_dropout_mask(mask.data_ptr(), n, seed, offset, keep, _st()) == 0          # aligned: the 16-byte path
    assert torch.equal(_bits(mask[:n]), _bits(m)) and bool((mask[n:] == -7.0).all())
    frac = float((mask[:n] != 0).double().mean())
    bound = 5 * (0.16 / n) ** 0.5
    print("kept fraction %.6f (0.8 +- %.1e)" % (frac, bound))
    assert abs(frac - 0.8) <= bound
    g = torch.Generator(device=DEV).manual_seed(3)
    data = torch.randn(n + 4, generator=g, device=DEV)
    for shift in (0, 1):
        a, b = data.clone(), data.clone()
        assert lib.hgt_dropout_apply(a.data_ptr() + 4 * shift, n, seed, offset, keep, _st()) == 0
        assert lib.hgt_mul_inplace(b.data_ptr() + 4 * shift, mask.data_ptr(), n, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a[shift + n:]), _bits(data[shift + n:]))


# -- graphs and layers ---------------------------------------------------------------------------------------------------------
def _square_graph(name):
    """(T, R, H, d, N, NQ, x, nt, ei, et, tm): every type has rows, every node a known type."""
    if name == "items_3k":            # the gather passes take the item-parallel hgt_edge_spmm_items
        T, R, H, d, N, E = 3, 5, 4, 64, 3000, 20000
    elif name == "sub_tile_70k":      # ... the sub-tile hgt_edge_spmm
        T, R, H, d, N, E = 3, 5, 8, 256, 70000, 300000
    else:
        raise KeyError(name)
    dp = _lib.layout_for(d, H).d_pad
    assert all(spmm_takes_items(N, E, R, ld, col) == (name == "items_3k") for ld, col in ((dp, 0), (3 * dp, 0), (3 * dp, dp), (3 * dp, 2 * dp)))
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=N + d)
    return T, R, H, d, N, N, x, nt, ei, et, tm


def _graph(name):
    if name == "rect_c1":             # NQ = 1300 of N = 2000: the rectangular step of a destination partition
        T, R, H, d, N, NQ, norm, rte, x, nt, ei, et, tm = PT._rect_graph("c1_rect")
        return T, R, H, d, N, NQ, x, nt, ei, et, tm
    return _square_graph(name)


def _layer(cls, graph, p, seed=71, **kw):
    T, R, H, d = graph[:4]
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=seed, dense=cls is DenseHGTConv)
    layer = cls(d, d, T, R, H, p, True, True, **kw)
    layer.load_state_dict(sd)
    return layer.to(DEV).train(), sd


def _step(layer, graph, gout, retain=False):
    """One training step: (out, {slot: gradient}) with x and every parameter among the slots."""
    T, R, H, d, N, NQ, x, nt, ei, et, tm = graph
    xd = x.to(DEV).requires_grad_(True)
    layer.zero_grad(set_to_none=True)
    GraphPlan.clear_cache()
    out = layer(xd, nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV), n_q_rows=NQ if NQ < N else None)
    out.backward(gout, retain_graph=retain)
    torch.cuda.synchronize()
    grads = {"x": xd.grad.clone()}
    grads.update({k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None})
    if retain:      # a second backward through the same graph: everything is recomputed once more, the gradients add up
        out.backward(gout)
        torch.cuda.synchronize()
        twice = {"x": xd.grad.clone()}
        twice.update({k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None})
        return out.detach().clone(), grads, twice
    return out.detach().clone(), grads


# -- 3. the promise the mode rests on ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["items_3k", "sub_tile_70k", "rect_c1"])
def test_project_run_twice_gives_the_same_bits(name, precision):
    graph = _graph(name)
    T, R, H, d, N, NQ, x, nt, ei, et, tm = graph
    layer, _ = _layer(HGTConv, graph, 0.0, precision=precision)
    plan = GraphPlan(nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV), T, R, n_q_rows=NQ if NQ < N else None)
    step = _Step(layer, plan, _lib.layout_for(d, H))
    p = SimpleNamespace(**layer._pack_parameters())
    xd = x.to(DEV)
    a = step.project(xd, p)
    junk = torch.randn(1 << 20, device=DEV)                       # other work in between, another address for the second result
    b = step.project(xd, p)
    torch.cuda.synchronize()
    assert a.shape == (NQ + 2 * N, step.dp) and a.data_ptr() != b.data_ptr() and junk.numel()
    assert torch.equal(_bits(a), _bits(b))
    # ... and a_linear (+ the counter-based dropout), the other step the backward runs again
    agg = torch.randn(NQ, step.dp, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    from pyhgt_amd.autograd import _DropSite
    site = _DropSite(2 ** 63 + 5, 1 << 40, 0.8)
    t1, t2 = step.a_linear(agg, p, site, gelu=True), step.a_linear(agg, p, site, gelu=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(t1), _bits(t2)) and bool((t1 == 0).any())


# -- 4. without dropout the two modes are the same function, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("cls", [HGTConv, DenseHGTConv], ids=["hgt", "dense"])
@pytest.mark.parametrize("name", ["items_3k", "sub_tile_70k", "rect_c1"])
def test_recompute_gives_the_bits_of_the_default_mode_without_dropout(name, cls):
    graph = _graph(name)
    d, NQ = graph[3], graph[5]
    gout = torch.randn(NQ, d, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV)
    res = {}
    for recompute in (False, True):
        layer, _ = _layer(cls, graph, 0.0, deterministic=True, recompute=recompute, keep_att=True)
        assert layer.training and layer.recompute is recompute
        res[recompute] = _step(layer, graph, gout, retain=True) + (layer.att.clone(),)
        if recompute:
            assert layer.last_dropout_state is None                # no dropout site was applied
    (o0, g0, t0, a0), (o1, g1, t1, a1) = res[False], res[True]
    assert o0.shape == (NQ, d) and torch.equal(_bits(o0), _bits(o1)) and torch.equal(_bits(a0), _bits(a1))
    names = {k for k, _ in layer.named_parameters() if k != "emb.emb.weight"} | {"x"}
    assert set(g0) == set(g1) >= names
    for k in g0:
        assert torch.equal(_bits(g0[k]), _bits(g1[k])), "%s differs between the modes" % k
        assert torch.equal(_bits(t0[k]), _bits(t1[k])), "%s differs between the modes after a second backward" % k
        assert bool(torch.isfinite(g1[k]).all())
    assert bool((t1["x"] - 2 * g1["x"]).abs().max() <= 1e-6 * g1["x"].abs().max())


# -- 5. dropout on: the oracle with the masks of the layer's seed ---------------------------------------------------------------
@pytest.mark.parametrize("conv", ["hgt", "dense"])
def test_dropout_gradients_match_the_oracle_with_the_masks_of_the_seed(conv, monkeypatch):
    """The graph, parameters and bounds of test_backward_gpu.test_dropout_gradients_match_the_oracle_with_the_drawn_masks at
    p = 0.2; the masks come from hgt_dropout_mask at layer.last_dropout_state instead of from torch.bernoulli."""
    dense = conv == "dense"
    p = 0.2
    T, R, H, d, N, E = 3, 4, 4, 64, 2000, 10000
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=51, dense=dense)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=52, sorted_types=False)
    nt = nt.clone()
    nt[::17] = T + 1
    layer = (DenseHGTConv if dense else HGTConv)(d, d, T, R, H, p, True, True, keep_att=True, recompute=True)
    layer.load_state_dict(sd)
    layer = layer.to(DEV).train()

    def no_bernoulli(*a, **k):
        raise AssertionError("the recompute mode draws no torch.bernoulli mask")

    monkeypatch.setattr(torch, "bernoulli", no_bernoulli)
    gout = torch.randn(N, d, generator=torch.Generator().manual_seed(53))
    xd = x.to(DEV).requires_grad_(True)
    GraphPlan.clear_cache()
    torch.manual_seed(2024)
    out = layer(xd, nt.to(DEV), ei.to(DEV), et.to(DEV), tm.to(DEV))
    out.backward(gout.to(DEV))
    torch.cuda.synchronize()
    monkeypatch.undo()
    seed, keep, offsets = layer.last_dropout_state
    assert isinstance(seed, int) and 0 <= seed < 2 ** 64 and keep == 1.0 - p
    assert offsets == ((0, 1 << 40) if dense else (0,))
    masks = [_mask(N * d, seed, off, keep).view(N, d).cpu() for off in offsets]
    assert all(0.75 < float((m != 0).float().mean()) < 0.85 for m in masks)          # keep probability 0.8
    assert all(set(m.unique().tolist()) == {0.0, float(np.float32(1) / np.float32(keep))} for m in masks)
    if dense:
        assert not torch.equal(masks[0], masks[1])
    dm = (masks[0], masks[1] if dense else None)
    fwd, att = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, use_norm=True, dense=dense, drop_masks=dm, return_att=True)
    assert (out.detach().cpu().double() - fwd).abs().max().item() < 1e-4
    assert layer.att is not None and (layer.att.cpu().double() - att).abs().max().item() < 1e-5      # keep_att under grad
    ref = O.backward_reference(sd, T, R, H, x, nt, ei, et, tm, gout, use_norm=True, dense=dense, drop_masks=dm)
    worst = BG._grads_close("x", xd.grad, ref["x"])
    for k, prm in layer.named_parameters():
        if k == "emb.emb.weight" and prm.grad is None:
            continue
        assert prm.grad is not None, k
        worst = max(worst, BG._grads_close(k, prm.grad, ref[k]))
    print("recompute dropout %s p=%.1f: worst relative gradient error %.2e" % (conv, p, worst))


# -- 6. a seeded step repeats --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [HGTConv, DenseHGTConv], ids=["hgt", "dense"])
def test_seeded_deterministic_step_repeats_bit_for_bit(cls):
    graph = _graph("items_3k")
    d, NQ = graph[3], graph[5]
    layer, _ = _layer(cls, graph, 0.2, deterministic=True, recompute=True)
    gout = torch.randn(NQ, d, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV)
    runs, states = [], []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        runs.append(_step(layer, graph, gout))
        states.append(layer.last_dropout_state)
    assert states[0] == states[1] and states[0][0] != states[2][0]
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and not torch.equal(runs[0][0], runs[2][0])
    assert set(runs[0][1]) == set(runs[1][1]) and len(runs[0][1]) > 10
    for k in runs[0][1]:
        assert torch.equal(_bits(runs[0][1][k]), _bits(runs[1][1][k])), "%s differs between two seeded runs" % k
    assert bool((runs[0][0] != 0).any())


def test_the_default_mode_calls_no_dropout_kernel_and_the_mode_calls_both(monkeypatch):
    lib = _lib.load()
    called = []
    for n in ("hgt_dropout_mask", "hgt_dropout_apply", "hgt_mul_inplace"):
        real = getattr(lib, n)
        monkeypatch.setattr(lib, n, (lambda *a, _n=n, _r=real: (called.append(_n), _r(*a))[1]))
    graph = _graph("items_3k")
    gout = torch.ones(graph[5], graph[3], device=DEV)
    layer, _ = _layer(DenseHGTConv, graph, 0.2)
    _step(layer, graph, gout)
    assert called == ["hgt_mul_inplace"] * 2 and layer.last_dropout_state is None
    del called[:]
    pyhgt_amd.set_recompute(layer)
    _step(layer, graph, gout)
    assert called == ["hgt_dropout_apply"] * 2 + ["hgt_dropout_mask"] * 2
    del called[:]
    layer.eval()                                                    # the differentiable path in eval mode: no dropout site at all
    _step(layer, graph, gout)
    assert called == [] and layer.last_dropout_state is None


# -- 7. memory -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [HGTConv, DenseHGTConv], ids=["hgt", "dense"])
def test_forward_keeps_less_memory(cls):
    """Growth of torch.cuda.memory_allocated() across a training forward, only `out` kept: smaller with recompute=True by the bytes
    of Q|K|V [(NQ + 2N) dp] and of two [NQ, dout] arrays (HGTConv: the a_linear output and its mask; DenseHGTConv: two masks),
    less 4 096 bytes for the allocator's rounding."""
    T, R, H, d, N, E, p = 3, 4, 8, 256, 8192, 65536, 0.2
    dp = _lib.layout_for(d, H).d_pad
    x, nt, ei, et, tm = [t.to(DEV) for t in synthetic_typed_graph(N, E, d, T, R, seed=9)]
    plan = GraphPlan(nt, ei, et, tm, T, R)
    gout = torch.ones(N, d, device=DEV)
    growth, requested = {}, {}
    asked = lambda: torch.cuda.memory_stats()["requested_bytes.all.current"]
    for recompute in (False, True):
        layer = cls(d, d, T, R, H, p, True, True, recompute=recompute).to(DEV).train()
        xd = x.clone().requires_grad_(True)
        # both modes start from the allocator state of a fresh process: memory_allocated() counts whole blocks, and a tensor that
        # lands in a cached block of an earlier test (up to 1 MiB larger: such a remainder is not split off) would count for more
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        layer(xd, nt, ei, et, tm, plan=plan).backward(gout)        # warm-up: the derived plans, the allocator's pools
        layer.zero_grad(set_to_none=True)
        xd.grad = None
        layer.att = None
        torch.cuda.synchronize()
        before, asked_before = torch.cuda.memory_allocated(), asked()
        out = layer(xd, nt, ei, et, tm, plan=plan)
        layer.att = None
        torch.cuda.synchronize()
        growth[recompute], requested[recompute] = torch.cuda.memory_allocated() - before, asked() - asked_before
        out.backward(gout)
        del out, layer, xd
        torch.cuda.synchronize()
    need = ((N + 2 * N) * dp + 2 * N * d) * 4 - 4096
    print("forward keeps %d bytes by default, %d with recompute: %d fewer (bound %d)" % (growth[False], growth[True],
                                                                                         growth[False] - growth[True], need))
    print("bytes asked of the allocator: %d by default, %d with recompute" % (requested[False], requested[True]))
    assert need == 41943040 - 4096
    assert growth[False] - growth[True] >= need


# -- 8. end to end -------------------------------------------------------------------------------------------------------------
def test_two_layer_gnn_under_set_recompute_lowers_its_loss():
    T, R, H, in_dim, d, N, E, n_cls = 3, 4, 4, 37, 64, 1200, 8000, 5
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, in_dim, T, R, seed=21)
    torch.manual_seed(1)
    gnn = GNN(in_dim, d, T, R, H, 2, dropout=0.2, conv_name="hgt", prev_norm=True, last_norm=True, use_RTE=True).to(DEV).train()
    head = Classifier(d, n_cls).to(DEV).train()
    model = pyhgt_amd.set_recompute(torch.nn.ModuleList([gnn, head]))
    assert all(gc.base_conv.recompute for gc in gnn.gcs)
    opt = torch.optim.AdamW(model.parameters(), lr=3e-3)
    y = torch.randint(0, n_cls, (200,)).to(DEV)
    dev = [t.to(DEV) for t in (x, nt, tm, ei, et)]
    losses, seeds = [], []
    GraphPlan.clear_cache()
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.nll_loss(head(gnn(*dev)[:200]), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        seeds += [gc.base_conv.last_dropout_state[0] for gc in gnn.gcs]
    print("losses under set_recompute: %s" % " ".join("%.4f" % v for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert len(set(seeds)) == len(seeds) == 20                      # one seed per layer call
