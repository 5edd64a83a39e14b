"""CPU tests of pyhgt_amd.optim: the float64 rule np_adamw_step against torch.optim.AdamW + clip_grad_norm_ in float64, the chunk table of
the kernels, state-dict interchange with torch.optim.AdamW, and the rejections.  No kernel runs here."""
import copy

import numpy as np
import pytest
import torch

import pyhgt_amd
from pyhgt_amd import _lib, AdamW, np_adamw_step
from pyhgt_amd.optim import chunk_table

SHAPES = [(7,), (3, 4), (5,), (6,), (2, 2)]
GROUPS = [dict(params=[0, 1, 2], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip=True),
          dict(params=[3, 4], lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1, clip=False)]
MAX_NORM = 5.0
NONE_AT = (1, 1)                     # (step, tensor): this tensor has no gradient at this step (the second of three)


def make_case(kind, seed=0):
    """-> (params, [grads of step 0, 1, 2]); kind: the norm of the clipped group's gradients against MAX_NORM"""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(s) for s in SHAPES]
    steps = []
    for t in range(3):
        grads = [rng.standard_normal(s) for s in SHAPES]
        clipped = [i for i in GROUPS[0]["params"] if (t, i) != NONE_AT]
        norm = np.sqrt(sum((grads[i] ** 2).sum() for i in clipped))
        if kind == "below":
            for i in clipped:
                grads[i] *= 0.3 * MAX_NORM / norm
        elif kind == "above":
            for i in clipped:
                grads[i] *= 40 * MAX_NORM / norm
        elif kind == "exact":                                                     # 3-4-5: a norm of exactly MAX_NORM in any precision
            for i in clipped:
                grads[i][...] = 0
            grads[0][t], grads[2][t + 1] = 3.0, -4.0
        elif kind == "zero":
            for i in clipped:
                grads[i][...] = 0
        else:
            assert kind == "inf"
            if t == 1:
                grads[2][3] = np.inf
        if (t, NONE_AT[1]) == NONE_AT:
            grads[NONE_AT[1]] = None
        steps.append(grads)
    return params, steps


def torch_chain(params, grad_steps, maximize, dtype=torch.float64, foreach=False):
    """torch.optim.AdamW + clip_grad_norm_ on the CPU -> per step (params, exp_avg, exp_avg_sq, step counts, norm) as float64 arrays"""
    P = [torch.nn.Parameter(torch.from_numpy(p).to(dtype).clone()) for p in params]
    groups = [dict({k: v for k, v in g.items() if k != "clip"}, params=[P[i] for i in g["params"]]) for g in GROUPS]
    opt = torch.optim.AdamW(groups, maximize=maximize, foreach=foreach)
    out = []
    for grads in grad_steps:
        for p, g in zip(P, grads):
            p.grad = None if g is None else torch.from_numpy(g).to(dtype).clone()
        norm = torch.nn.utils.clip_grad_norm_([P[i] for g in GROUPS if g["clip"] for i in g["params"]], MAX_NORM, foreach=foreach)
        opt.step()
        state = [opt.state.get(p, {}) for p in P]
        out.append(([p.detach().double().numpy().copy() for p in P],
                    [s["exp_avg"].double().numpy().copy() if s else np.zeros(p.shape) for s, p in zip(state, P)],
                    [s["exp_avg_sq"].double().numpy().copy() if s else np.zeros(p.shape) for s, p in zip(state, P)],
                    [int(s["step"].item()) if s else 0 for s in state], float(norm)))
    return out


def rule_chain(params, grad_steps, maximize):
    groups = [dict(g, maximize=maximize) for g in GROUPS]
    p, m, v, s = params, [np.zeros(x.shape) for x in params], [np.zeros(x.shape) for x in params], [0] * len(params)
    out = []
    for grads in grad_steps:
        p, m, v, s, norm = np_adamw_step(p, grads, m, v, s, groups, MAX_NORM)
        out.append((p, m, v, s, norm))
    return out


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("kind", ["below", "above", "exact", "zero"])
def test_rule_equals_torch_in_float64(kind, maximize):
    """the same rule in another operation order: 2^-45 (|p| + |delta|) per element (float64 has 2^-53; torch forms m by lerp, the norm
    from per-tensor norms and p by addcdiv)"""
    params, grad_steps = make_case(kind)
    want, got = torch_chain(params, grad_steps, maximize), rule_chain(params, grad_steps, maximize)
    old = params
    tol = 2.0 ** -45
    for t, (w, g) in enumerate(zip(want, got)):
        assert w[3] == g[3], "step counts"
        assert abs(w[4] - g[4]) <= tol * w[4]
        if kind == "exact":
            assert g[4] == MAX_NORM
        for i in range(len(params)):
            delta = np.abs(w[0][i] - old[i])
            assert (np.abs(w[0][i] - g[0][i]) <= tol * (np.abs(old[i]) + delta)).all(), (t, i)
            gi = grad_steps[t][i]
            scale = 1.0 if gi is None else np.abs(gi)
            assert (np.abs(w[1][i] - g[1][i]) <= tol * (np.abs(w[1][i]) + scale)).all(), (t, i)
            assert (np.abs(w[2][i] - g[2][i]) <= tol * (np.abs(w[2][i]) + scale ** 2)).all(), (t, i)
        old = w[0]
    t, i = NONE_AT                                                                # skipped entirely: no decay, no state change, no count
    before = (params[i], np.zeros(SHAPES[i]), np.zeros(SHAPES[i])) if t == 0 else tuple(got[t - 1][k][i] for k in range(3))
    assert all(np.array_equal(got[t][k][i], before[k]) for k in range(3)) and got[t][3][i] == got[t][3][0] - 1
    if kind == "zero":                                                            # only the decay moves a clipped tensor
        assert np.allclose(got[0][0][0], params[0] * (1 - 1e-3 * 1e-2), rtol=1e-15, atol=0)


@pytest.mark.parametrize("maximize", [False, True])
def test_rule_and_torch_agree_on_the_pattern_of_an_infinite_gradient(maximize):
    params, grad_steps = make_case("inf")
    want, got = torch_chain(params, grad_steps, maximize), rule_chain(params, grad_steps, maximize)
    for w, g in zip(want, got):
        assert np.isinf(w[4]) == np.isinf(g[4]) and np.isnan(w[4]) == np.isnan(g[4])
        for k in range(3):
            for a, b in zip(w[k], g[k]):
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
    assert np.isinf(got[1][4]) and np.isnan(got[1][0][2][3]) and np.isfinite(got[1][0][0]).all()
    assert all(np.isfinite(got[2][0][i]).all() for i in GROUPS[1]["params"])      # the unclipped group never sees it


def test_rule_modifies_nothing_in_place():
    params, grad_steps = make_case("above")
    keep = copy.deepcopy((params, grad_steps))
    rule_chain(params, grad_steps, False)
    assert all(np.array_equal(a, b) for a, b in zip(params, keep[0]))
    assert all(a is None and b is None or np.array_equal(a, b) for x, y in zip(grad_steps, keep[1]) for a, b in zip(x, y))


def test_chunk_constant_is_one_number_in_header_binding_and_library():
    import ctypes
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hgt_hip.h")).read()
    got = ctypes.c_int32()
    assert _lib.load().hgt_optim_constants(ctypes.byref(got)) == 0
    assert got.value == _lib.OPTIM_CHUNK == int(re.search(r"#define HGT_OPTIM_CHUNK (\d+)", header).group(1))
    assert _lib.load().hgt_optim_constants(None) == -1


def test_state_dict_leaves_out_a_parameter_without_state():
    """Optimizer.state is a defaultdict: an entry that a read planted for a parameter without a gradient is not a state"""
    params = [torch.nn.Parameter(torch.zeros(3)) for _ in range(2)]
    opt = AdamW(params)
    opt.state[params[0]].update(step=4, exp_avg=torch.ones(3), exp_avg_sq=torch.ones(3))
    assert opt.state[params[1]] == {}
    sd = opt.state_dict()
    assert list(sd["state"]) == [0] and float(sd["state"][0]["step"]) == 4
    torch.optim.AdamW(params).load_state_dict(sd)


def test_chunk_table_covers_every_element_once():
    C = _lib.OPTIM_CHUNK
    assert C == 4096
    numels = [1, 3, 4, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5]
    row, first = chunk_table(numels)
    assert row.dtype == np.int32 and first.dtype == np.int64 and row.shape == first.shape
    assert (np.diff(row) >= 0).all()                                              # parameter order
    covered = [np.zeros(n, dtype=np.int64) for n in numels]
    for r, f in zip(row, first):
        assert 0 <= r < len(numels) and 0 <= f < numels[r] and f % C == 0
        covered[r][f:min(f + C, numels[r])] += 1                                  # a chunk ends with its tensor: none spans two
    assert all((c == 1).all() for c in covered)
    assert len(row) == sum(-(-n // C) for n in numels)
    for r in range(len(numels)):                                                  # a tensor's chunks in element order
        assert (np.diff(first[row == r]) == C).all()
    assert len(chunk_table([])[0]) == 0 and len(chunk_table([0, 0])[0]) == 0
    assert chunk_table([4, 0, 4])[0].tolist() == [0, 2]


def _stepped_torch(params, n_steps=2):
    opt = torch.optim.AdamW([dict(params=params[:2], lr=2e-3), dict(params=params[2:], weight_decay=0.2)])
    g = torch.Generator().manual_seed(3)
    for _ in range(n_steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def _same_state(a, b):
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        sa, sb = a["state"][k], b["state"][k]
        assert sa.keys() == sb.keys() == {"step", "exp_avg", "exp_avg_sq"}
        assert torch.is_tensor(sa["step"]) and torch.is_tensor(sb["step"]) and sa["step"].dtype == sb["step"].dtype == torch.float32
        assert sa["step"].device.type == "cpu" and float(sa["step"]) == float(sb["step"])
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


def test_state_dicts_move_between_this_class_and_torch():
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    theirs = _stepped_torch(params)
    sd = theirs.state_dict()
    ours = AdamW([dict(params=params[:2]), dict(params=params[2:], clip=False)], max_norm=0.5)
    assert ours.state_dict()["state"] == {}
    ours.load_state_dict(sd)
    assert all(isinstance(ours.state[p]["step"], int) and ours.state[p]["step"] == 2 for p in params)
    assert [g["lr"] for g in ours.param_groups] == [2e-3, 1e-3] and [g["weight_decay"] for g in ours.param_groups] == [1e-2, 0.2]
    assert [g["clip"] for g in ours.param_groups] == [True, False]                # torch's groups carry no `clip`: ours keep theirs
    back = ours.state_dict()
    _same_state(sd, back)
    assert set(sd["param_groups"][0]) | {"clip"} == set(back["param_groups"][0])
    fresh = torch.optim.AdamW([dict(params=params[:2]), dict(params=params[2:])])
    fresh.load_state_dict(back)
    _same_state(sd, fresh.state_dict())
    assert fresh.param_groups[0]["decoupled_weight_decay"] is True and fresh.param_groups[0]["lr"] == 2e-3
    for p in params:                                                              # and torch goes on stepping from it
        p.grad = torch.ones_like(p)
    fresh.step()
    assert all(float(fresh.state[p]["step"]) == 3 for p in params)
    again = AdamW([dict(params=params[:2]), dict(params=params[2:])])
    again.load_state_dict(copy.deepcopy(back))
    _same_state(again.state_dict(), back)


def test_rejections_name_the_parameter():
    w = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        AdamW([w], amsgrad=True)
    with pytest.raises(TypeError, match=r"parameter 1 of group 0 \(shape \(2,\)\).*float16"):
        AdamW([w, torch.nn.Parameter(torch.zeros(2, dtype=torch.float16))])
    with pytest.raises(TypeError, match="parameter 'head.bias'.*float16"):
        AdamW([("body.weight", w), ("head.bias", torch.nn.Parameter(torch.zeros(2, dtype=torch.float16)))])
    with pytest.raises(ValueError, match="max_norm"):
        AdamW([w], max_norm=-1.0)
    emb = torch.nn.Embedding(5, 3, sparse=True)
    opt = AdamW([w, emb.weight])
    emb(torch.tensor([1, 2])).sum().backward()
    assert emb.weight.grad.is_sparse
    with pytest.raises(RuntimeError, match=r"parameter 1 of group 0 \(shape \(5, 3\)\) has a sparse gradient"):
        opt.step()
    bad = _stepped_torch([torch.nn.Parameter(torch.zeros(3)) for _ in range(3)]).state_dict()
    bad["param_groups"][0]["amsgrad"] = True
    mine = [torch.nn.Parameter(torch.zeros(3)) for _ in range(3)]
    with pytest.raises(NotImplementedError, match="amsgrad"):
        AdamW([dict(params=mine[:2]), dict(params=mine[2:])]).load_state_dict(bad)


def test_step_on_cpu_tensors_raises_the_documented_sentence():
    w = torch.nn.Parameter(torch.zeros(4, 3))
    opt = AdamW([w], max_norm=1.0)
    w.grad = torch.ones_like(w)
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU tensor; np_adamw_step is the definition"):
        opt.step()
    assert not w.detach().any() and opt.total_norm is None and pyhgt_amd.AdamW is AdamW
