"""The optimizer kernels (csrc/hgt_optim.hip) behind pyhgt_amd.AdamW on the GPU against the float64 rule np_adamw_step.

Every step is compared on its own: the rule and torch's float32 CPU chain (AdamW(foreach=False) + clip_grad_norm_) both start from the
state the device holds before the step, so the three steps are chained through the device's own p, exp_avg and exp_avg_sq.

Gates (derived, not chosen; float32 device results against the float64 rule):
  p           per element 4 x max(E_torch, 2^-23 (|p_old| + |delta|)): E_torch is the error of torch's own float32 CPU chain on the same
              inputs against the rule -- another operation order is as legitimate as torch's -- and the floor keeps elements alive on
              which torch happens to be exact: p_new = p_old decay - delta is two float32 roundings of magnitudes |p_old| and |delta|
  exp_avg     the same with the floor 2^-23 (|b1 m_old| + |(1 - b1) g|), the two magnitudes that are added
  exp_avg_sq  the same with the floor 2^-23 (b2 v_old + (1 - b2) g^2)
  total_norm  4 x max(E_torch, 2^-23 norm)
Measured on an MI355X (pytest -s prints them), the worst error over every layout and step of the first test with the gate of that
element: p 2.7e-07 under 1.3e-06, exp_avg 5.3e-08 under 2.4e-07, exp_avg_sq 1.4e-08 under 6.2e-08, total_norm (about 144) 3.7e-06
under 6.9e-05.  Without max_norm on gradients of scale 30: p 2.3e-07 under 1.5e-06, exp_avg 1.1e-06 under 1.1e-05, exp_avg_sq
1.2e-05 under 6.2e-05."""
import copy

import numpy as np
import pytest
import torch

import pyhgt_amd
from pyhgt_amd import _lib, AdamW, Classifier, GNN, GraphPlan, np_adamw_step
from pyhgt_amd.synth import synthetic_typed_graph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = _lib.OPTIM_CHUNK
EPS32 = 2.0 ** -23
NUMELS = [1, 3, 4, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5]
N_T = 2 * len(NUMELS)                # the sizes once in a clipped group, once in an unclipped one
HYPER = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, clip=True),
         dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1, clip=False)]
MAX_NORM = 1.0
SCALES = (1.0, 1e-3, 1.0)            # the clipped group's norm is about 130, 0.13, 130: clipped, not clipped, clipped
WORST = {"p": (0.0, 0.0), "m": (0.0, 0.0), "v": (0.0, 0.0), "norm": (0.0, 0.0)}


def groups_of(maximize=False, hyper=HYPER):
    half = N_T // 2
    return [dict(hyper[0], params=list(range(half)), maximize=maximize), dict(hyper[1], params=list(range(half, N_T)), maximize=maximize)]


def place(a, odd):
    """a host vector on the device in the middle of NaN guards -> (view, whole): one float off 16-byte alignment (odd) or on it"""
    lead = 1 if odd else 4
    whole = torch.full((a.size + lead + 3,), float("nan"), dtype=torch.float32)
    whole[lead:lead + a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    whole = whole.to(DEV)
    view = whole[lead:lead + a.size]
    assert view.data_ptr() % 16 == (4 if odd else 0)
    return view, whole


def guards_intact(view, whole):
    lead = (view.data_ptr() - whole.data_ptr()) // 4
    return bool(torch.isnan(whole[:lead]).all()) and bool(torch.isnan(whole[lead + view.numel():]).all())


def is_odd(layout, i, which):
    """tensor i has `which` (p, g, m, v) one float off alignment: layout = that letter, 'all', 'turns' (each in turn) or 'contiguous'"""
    return layout == "all" or layout == which or (layout == "turns" and "pgmv"[i % 4] == which)


def torch32_step(p, g, m, v, steps, groups, max_norm):
    """one step of torch's float32 CPU chain from this state -> (p, m, v, norm) as float64"""
    P = [torch.nn.Parameter(torch.from_numpy(np.array(a, dtype=np.float32))) for a in p]
    opt = torch.optim.AdamW([dict(params=[P[i] for i in grp["params"]], lr=grp["lr"], betas=grp["betas"], eps=grp["eps"],
                                  weight_decay=grp["weight_decay"], maximize=grp.get("maximize", False)) for grp in groups], foreach=False)
    for i, q in enumerate(P):
        if steps[i] > 0:
            opt.state[q] = dict(step=torch.tensor(float(steps[i])), exp_avg=torch.from_numpy(np.array(m[i], dtype=np.float32)),
                                exp_avg_sq=torch.from_numpy(np.array(v[i], dtype=np.float32)))
        q.grad = None if g[i] is None else torch.from_numpy(np.array(g[i], dtype=np.float32))
    norm = None
    if max_norm is not None:
        norm = float(torch.nn.utils.clip_grad_norm_([P[i] for grp in groups if grp.get("clip", True) for i in grp["params"]], max_norm,
                                                    foreach=False))
    opt.step()
    zero = lambda i: np.zeros(p[i].shape)
    return ([q.detach().double().numpy() for q in P],
            [opt.state[q]["exp_avg"].double().numpy() if q in opt.state and opt.state[q] else zero(i) for i, q in enumerate(P)],
            [opt.state[q]["exp_avg_sq"].double().numpy() if q in opt.state and opt.state[q] else zero(i) for i, q in enumerate(P)], norm)


def reference(p, g, m, v, steps, groups, max_norm):
    """the rule's step from this float32 state and the gates of the module docstring -> (want, gates), each (p, m, v, norm)"""
    want = np_adamw_step(p, g, m, v, steps, groups, max_norm)
    t32 = torch32_step(p, g, m, v, steps, groups, max_norm)
    gates = ([], [], [])
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (want[4] + 1e-6))
    for grp in groups:
        b1, b2 = grp["betas"]
        for i in grp["params"]:
            if g[i] is None:
                for k in range(3):
                    gates[k].append(np.zeros(p[i].shape))
                continue
            gi = np.asarray(g[i], dtype=np.float64) * (coef if grp.get("clip", True) and max_norm is not None else 1.0)
            p_old, m_old, v_old = (np.asarray(a[i], dtype=np.float64) for a in (p, m, v))
            delta = np.abs(want[0][i] - p_old * (1.0 - grp["lr"] * grp["weight_decay"]))
            floors = (EPS32 * (np.abs(p_old) + delta), EPS32 * (np.abs(b1 * m_old) + np.abs((1 - b1) * gi)),
                      EPS32 * (b2 * v_old + (1 - b2) * gi * gi))
            for k in range(3):
                gates[k].append(4 * np.fmax(np.abs(t32[k][i] - want[k][i]), floors[k]))
    order = [i for grp in groups for i in grp["params"]]
    gates = tuple([gk[order.index(i)] for i in range(len(order))] for gk in gates)
    norm_gate = None if max_norm is None else 4 * max(abs(t32[3] - want[4]), EPS32 * want[4])
    return want, gates + (norm_gate,)


class Bench:
    """N_T tensors in two groups under one AdamW, each of p, g, m, v placed by the layout; the host keeps nothing but what it downloads"""

    def __init__(self, layout, seed, maximize=False, max_norm=MAX_NORM, keep=None):
        self.rng = np.random.default_rng(seed)
        self.layout, self.max_norm = layout, max_norm
        self.keep = list(range(N_T)) if keep is None else keep                   # the tensors this optimizer holds
        self.groups = groups_of(maximize)
        self.wholes = []
        p0 = [self.rng.standard_normal(NUMELS[i % len(NUMELS)]).astype(np.float32) for i in range(N_T)]
        self.P = {}
        for i in self.keep:
            view, whole = place(p0[i], is_odd(layout, i, "p"))
            self.P[i] = torch.nn.Parameter(view)
            self.wholes.append((view, whole))
        half = N_T // 2
        self.opt = AdamW([dict(HYPER[0], params=[self.P[i] for i in self.keep if i < half]),
                          dict(HYPER[1], params=[self.P[i] for i in self.keep if i >= half])], maximize=maximize, max_norm=max_norm)
        for i in self.keep:                                                       # the moments where the layout wants them
            zeros = np.zeros(p0[i].size, dtype=np.float32)
            mv, mw = place(zeros, is_odd(layout, i, "m"))
            vv, vw = place(zeros, is_odd(layout, i, "v"))
            self.opt.state[self.P[i]] = {"step": 0, "exp_avg": mv, "exp_avg_sq": vv}
            self.wholes += [(mv, mw), (vv, vw)]
        self.opt.invalidate()

    def draw(self, scale, none=()):
        return [None if i in none else (self.rng.standard_normal(NUMELS[i % len(NUMELS)]) * scale).astype(np.float32) for i in range(N_T)]

    def set_grads(self, grads):
        for i in self.keep:
            if grads[i] is None:
                self.P[i].grad = None
            else:
                view, whole = place(grads[i], is_odd(self.layout, i, "g"))
                self.P[i].grad = view
                self.wholes.append((view, whole))

    def state(self):
        """(p, m, v, steps) on the host as the device holds them; tensors this optimizer does not hold are None"""
        get = lambda t: t.detach().cpu().numpy().copy()
        st = lambda i: self.opt.state[self.P[i]]
        has = lambda i: i in self.P
        return ([get(self.P[i]) if has(i) else None for i in range(N_T)], [get(st(i)["exp_avg"]) if has(i) else None for i in range(N_T)],
                [get(st(i)["exp_avg_sq"]) if has(i) else None for i in range(N_T)], [st(i)["step"] if has(i) else None for i in range(N_T)])


def check_step(before, grads, after, norm, groups, max_norm, what):
    want, gates = reference(before[0], grads, before[1], before[2], before[3], groups, max_norm)
    assert after[3] == want[3]
    for k, name in enumerate("pmv"):
        worst, worst_gate = 0.0, 0.0
        for i in range(N_T):
            err = np.abs(after[k][i].astype(np.float64) - want[k][i])
            assert np.isfinite(after[k][i]).all()
            j = (err - gates[k][i]).argmax()
            if err.max() >= worst:
                worst, worst_gate = err.max(), gates[k][i][err.argmax()]
            assert (err <= gates[k][i]).all(), (what, name, i, j, err[j], gates[k][i][j])
        print("%s %s: worst error %.3e (its gate %.3e)" % (what, name, worst, worst_gate))
        if worst > WORST[name][0]:
            WORST[name] = (worst, worst_gate)
    if max_norm is not None:
        err = abs(float(norm) - want[4])
        print("%s total_norm %.6e: error %.3e (gate %.3e)" % (what, want[4], err, gates[3]))
        if err > WORST["norm"][0]:
            WORST["norm"] = (err, gates[3])
        assert err <= gates[3]


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("layout", ["contiguous", "turns", "p", "g", "m", "v", "all"])
def test_three_chained_steps_against_the_rule(layout, maximize):
    b = Bench(layout, seed=11, maximize=maximize)
    for t, scale in enumerate(SCALES):
        before, grads = b.state(), b.draw(scale)
        b.set_grads(grads)
        b.opt.step()
        assert b.opt.total_norm.device.type == "cuda" and b.opt.total_norm.dtype == torch.float32 and b.opt.total_norm.dim() == 0
        check_step(before, grads, b.state(), b.opt.total_norm.item(), b.groups, MAX_NORM, "%s step %d" % (layout, t + 1))
        for i in b.keep:                                                          # p.grad stays as backward left it
            assert np.array_equal(b.P[i].grad.cpu().numpy().view(np.uint32), grads[i].view(np.uint32))
    assert all(guards_intact(view, whole) for view, whole in b.wholes)            # nothing outside p, g, m, v was touched
    print("worst so far: " + ", ".join("%s %.3e under %.3e" % ((k,) + v) for k, v in WORST.items()))


def test_without_max_norm_nothing_is_clipped():
    b = Bench("turns", seed=12, max_norm=None)
    before, grads = b.state(), b.draw(30.0)
    b.set_grads(grads)
    b.opt.step()
    assert b.opt.total_norm is None
    check_step(before, grads, b.state(), None, b.groups, None, "no clip")


def bits(arrays):
    return [None if a is None else np.asarray(a).view(np.uint32) for a in arrays]


def same_bits(a, b, only=None):
    return all(np.array_equal(x, y) for i, (x, y) in enumerate(zip(bits(a), bits(b))) if (only is None or i in only) and x is not None and y is not None)


def test_a_tensor_without_a_gradient_is_skipped_entirely():
    skipped = [2, 5, 8, 9, 13, 19]                                                # small and multi-chunk tensors of both groups
    rest = [i for i in range(N_T) if i not in skipped]
    a, b = Bench("turns", seed=13, max_norm=None), Bench("turns", seed=13, max_norm=None, keep=rest)
    for t, none in enumerate(((), skipped, skipped)):
        before = a.state()
        grads = a.draw(1.0, none=none)
        b.draw(1.0)                                                               # (the same stream of draws)
        a.set_grads(grads), b.set_grads([None if i in skipped else grads[i] for i in range(N_T)])
        a.opt.step(), b.opt.step()
        after, other = a.state(), b.state()
        if none:
            assert all(same_bits(after[k], before[k], only=skipped) for k in range(3))
            assert all(after[3][i] == before[3][i] == 1 for i in skipped)
        assert all(after[3][i] == t + 1 for i in rest)
        assert all(same_bits(after[k], other[k], only=rest) for k in range(3))    # as if the skipped ones had never been there
    assert all(guards_intact(view, whole) for view, whole in a.wholes)


def test_a_non_finite_gradient_stays_in_the_clipped_group():
    a, clean = Bench("turns", seed=14), Bench("turns", seed=14)
    grads = a.draw(1.0)
    clean.draw(1.0)
    poisoned = copy.deepcopy(grads)
    poisoned[7][100] = np.inf                                                     # one element of a clipped tensor
    before = a.state()
    a.set_grads(poisoned), clean.set_grads(grads)
    a.opt.step(), clean.opt.step()
    got, ok = a.state(), clean.state()
    want = np_adamw_step(before[0], poisoned, before[1], before[2], before[3], a.groups, MAX_NORM)
    assert np.isinf(want[4]) and np.isinf(a.opt.total_norm.item())
    half = N_T // 2
    for k in range(3):
        for i in range(N_T):
            assert np.array_equal(np.isnan(got[k][i]), np.isnan(want[k][i])) and np.array_equal(np.isinf(got[k][i]), np.isinf(want[k][i])), (k, i)
        assert same_bits(got[k], ok[k], only=range(half, N_T))                    # the unclipped group is untouched by it
    assert np.isnan(got[0][7][100]) and np.isfinite(np.delete(got[0][7], 100)).all()
    # with coef = 0 every finite clipped gradient is 0: only the decay moves those parameters
    assert np.array_equal(got[0][0], before[0][0] * np.float32(1.0 - 1e-3 * 1e-2))


@pytest.mark.parametrize("fresh_grads", [False, True])
def test_same_bits_twice(fresh_grads):
    """two optimizers over cloned tensors: identical p, m, v and norm after three steps -- also where one of them gets its gradients
    in newly allocated tensors every step (other pointers, other alignments of the allocation) and the other in place"""
    a, b = Bench("contiguous", seed=15), Bench("contiguous", seed=15)
    hold = []
    for t, scale in enumerate(SCALES):
        grads = a.draw(scale)
        b.draw(scale)
        a.set_grads(grads)
        if fresh_grads or t == 0:
            b.set_grads(grads)
            hold.append([b.P[i].grad for i in b.keep])                            # kept alive: the next step's get other addresses
        else:
            for i in b.keep:
                b.P[i].grad.copy_(torch.from_numpy(grads[i]))
        a.opt.step(), b.opt.step()
        assert a.opt.total_norm.cpu().numpy().view(np.uint32) == b.opt.total_norm.cpu().numpy().view(np.uint32)
        sa, sb = a.state(), b.state()
        assert all(same_bits(sa[k], sb[k]) for k in range(3)) and sa[3] == sb[3]


def test_the_16_byte_and_the_scalar_path_give_the_same_bits():
    """every tensor on 16 bytes against every one of p, g, m, v one float off: element i gets the same bits, and so does the norm"""
    a, b = Bench("contiguous", seed=18), Bench("all", seed=18)
    for scale in SCALES:
        grads = a.draw(scale)
        b.draw(scale)
        a.set_grads(grads), b.set_grads(grads)
        a.opt.step(), b.opt.step()
        assert a.opt.total_norm.cpu().numpy().view(np.uint32) == b.opt.total_norm.cpu().numpy().view(np.uint32)
        sa, sb = a.state(), b.state()
        assert all(same_bits(sa[k], sb[k]) for k in range(3)) and sa[3] == sb[3]
    assert all(guards_intact(view, whole) for view, whole in a.wholes + b.wholes)


def small_params(n=3):
    g = torch.Generator().manual_seed(19)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in ((5,), (C + 3,), (7, 3))[:n]]


def test_a_checkpoint_with_a_tensor_that_never_had_a_gradient():
    """a frozen tensor has no state, as in torch: state_dict() leaves it out, torch.optim.AdamW loads it, and it comes back"""
    P = small_params()
    opt = AdamW(P, max_norm=1.0)
    before = P[1].detach().clone()
    for _ in range(2):
        P[0].grad, P[2].grad = torch.ones_like(P[0]), torch.ones_like(P[2])
        opt.step()
    assert P[1] not in opt.state and torch.equal(P[1], before)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 2] and all(float(s["step"]) == 2 for s in sd["state"].values())
    theirs = torch.optim.AdamW(P, foreach=False)
    theirs.load_state_dict(sd)
    assert sorted(theirs.state_dict()["state"]) == [0, 2]
    back = AdamW(P, max_norm=1.0)
    back.load_state_dict(theirs.state_dict())
    assert P[1] not in back.state and [back.state[q]["step"] for q in (P[0], P[2])] == [2, 2]
    for q in (P[0], P[2]):
        assert torch.equal(back.state[q]["exp_avg"], opt.state[q]["exp_avg"]) and torch.equal(back.state[q]["exp_avg_sq"], opt.state[q]["exp_avg_sq"])
    for q in P:                                                                   # now the frozen one gets its first gradient
        q.grad = torch.ones_like(q)
    back.step()
    assert [back.state[q]["step"] for q in P] == [3, 1, 3] and not torch.equal(P[1], before)
    assert sorted(back.state_dict()["state"]) == [0, 1, 2]


def test_a_rejected_gradient_changes_nothing():
    """every gradient is checked before any state is made or any step count goes up"""
    P = small_params()
    opt = AdamW(P, max_norm=1.0)
    for q in P:
        q.grad = torch.ones_like(q)
    opt.step()
    keep = [q.detach().clone() for q in P]
    P[2].grad = torch.ones_like(P[2]).to_sparse()
    with pytest.raises(RuntimeError, match=r"parameter 2 of group 0 \(shape \(7, 3\)\) has a sparse gradient"):
        opt.step()
    torch.cuda.synchronize()
    assert [opt.state[q]["step"] for q in P] == [1, 1, 1] and all(torch.equal(a, b) for a, b in zip(P, keep))
    P[2].grad = torch.ones_like(P[2])
    opt.step()
    assert [opt.state[q]["step"] for q in P] == [2, 2, 2] and not any(torch.equal(a, b) for a, b in zip(P, keep))


def test_a_step_without_any_gradient_has_norm_zero():
    P = small_params()
    opt = AdamW(P, max_norm=1.0)
    for q in P:
        q.grad = torch.ones_like(q)
    opt.step()
    assert opt.total_norm.item() > 0
    keep = [q.detach().clone() for q in P]
    opt.zero_grad(set_to_none=True)
    opt.step()
    assert opt.total_norm.item() == 0 and all(torch.equal(a, b) for a, b in zip(P, keep)) and all(opt.state[q]["step"] == 1 for q in P)


def test_step_does_not_synchronise_the_host():
    b = Bench("turns", seed=16)
    b.set_grads(b.draw(1.0))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                                         # the mode is honoured by this build: .item() is caught
            torch.ones(1, device=DEV).item()
        for _ in range(2 * 4 + 1):                                                # first step (tables are built) and round the staging ring
            b.opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert b.opt.state[b.P[0]]["step"] == 9


# ---------------------------------------------------------------------------------------------------------------- with the model
def tiny_model(seed, deterministic=False):
    T, R, H, in_dim, d, n_cls = 3, 4, 2, 19, 32, 5
    torch.manual_seed(seed)
    gnn = GNN(in_dim, d, T, R, H, 2, dropout=0.0, prev_norm=True, last_norm=True, use_RTE=True)
    head = Classifier(d, n_cls)
    model = torch.nn.ModuleList([gnn, head]).to(DEV)
    if deterministic:
        pyhgt_amd.set_deterministic(model, True)
    return model


def tiny_graph():
    x, nt, ei, et, tm = synthetic_typed_graph(200, 800, 19, 3, 4, seed=31)
    return [t.to(DEV) for t in (x, nt, tm, ei, et)], torch.randint(0, 5, (50,), generator=torch.Generator().manual_seed(2)).to(DEV)


def make_opt(model):
    return AdamW([dict(params=list(model[0].parameters())), dict(params=list(model[1].parameters()), clip=False)], lr=1e-2, max_norm=0.5)


def train_step(model, opt, graph, y):
    model.train()
    opt.zero_grad(set_to_none=True)
    loss = torch.nn.functional.nll_loss(model[1](model[0](*graph)[:50]), y)
    loss.backward()
    opt.step()
    return loss


def test_eval_after_a_step_runs_on_the_new_weights():
    """the packed-weight caches of HGTConv / GNN are keyed on the parameters' version counters; the kernels write through raw pointers"""
    graph, y = tiny_graph()
    model = tiny_model(5)
    opt = make_opt(model)
    model.eval()
    with torch.no_grad():
        first = model[1](model[0](*graph)).clone()                                # fills the caches
    versions = [p._version for p in model.parameters()]
    train_step(model, opt, graph, y)
    assert all(p._version > v for p, v in zip(model.parameters(), versions) if p.grad is not None)
    model.eval()
    with torch.no_grad():
        got = model[1](model[0](*graph))
    fresh = tiny_model(6)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        want = fresh[1](fresh[0](*graph))
    assert not torch.equal(got, first)
    assert torch.equal(got, want)
    GraphPlan.clear_cache()                                                       # leave no device memory behind for later tests


def test_three_training_steps_repeat_bit_for_bit():
    graph, y = tiny_graph()
    runs = []
    for _ in range(2):
        GraphPlan.clear_cache()
        model = tiny_model(7, deterministic=True)
        opt = make_opt(model)
        losses = [train_step(model, opt, graph, y).item() for _ in range(3)]
        runs.append(([p.detach().clone() for p in model.parameters()], losses, opt.total_norm.clone()))
    assert runs[0][1] == runs[1][1] and torch.equal(runs[0][2], runs[1][2])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert runs[0][1][2] < runs[0][1][0]                                          # and it trains
    GraphPlan.clear_cache()


@pytest.mark.parametrize("direction", ["ours to torch", "torch to ours"])
def test_checkpoints_move_between_this_class_and_torch_on_the_device(direction):
    """two steps with one class, its state dict loaded into the other, one more step with the same gradients on both sides: the step
    counts and the moments arrived.  Ours is within the gate of the module docstring of the rule, and the two classes' results are
    within that same gate of each other."""
    rng = np.random.default_rng(17)
    groups = groups_of()
    p0 = [rng.standard_normal(NUMELS[i % len(NUMELS)]).astype(np.float32) for i in range(N_T)]
    half = N_T // 2

    def build(cls, **kw):
        P = [torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in p0]
        strip = (lambda h: {k: v for k, v in h.items() if k != "clip"}) if cls is torch.optim.AdamW else (lambda h: h)
        return P, cls([dict(strip(HYPER[0]), params=P[:half]), dict(strip(HYPER[1]), params=P[half:])], **kw)

    def step(P, opt, grads, clip):
        for q, g in zip(P, grads):
            q.grad = torch.from_numpy(g).to(DEV)
        if clip:
            torch.nn.utils.clip_grad_norm_(P[:half], MAX_NORM, foreach=False)
        opt.step()

    ours_first = direction == "ours to torch"
    PA, A = build(AdamW, max_norm=MAX_NORM) if ours_first else build(torch.optim.AdamW, foreach=False)
    PB, B = build(torch.optim.AdamW, foreach=False) if ours_first else build(AdamW, max_norm=MAX_NORM)
    for scale in SCALES[:2]:
        step(PA, A, [(rng.standard_normal(a.size) * scale).astype(np.float32) for a in p0], clip=not ours_first)
    B.load_state_dict(copy.deepcopy(A.state_dict()))
    with torch.no_grad():
        for qa, qb in zip(PA, PB):
            qb.copy_(qa)
    get = lambda t: t.detach().cpu().numpy().copy()
    before = ([get(q) for q in PA], [get(A.state[q]["exp_avg"]) for q in PA], [get(A.state[q]["exp_avg_sq"]) for q in PA], [2] * N_T)
    grads = [rng.standard_normal(a.size).astype(np.float32) for a in p0]
    step(PA, A, grads, clip=not ours_first)
    step(PB, B, grads, clip=ours_first)
    assert all(int(A.state[q]["step"]) == 3 for q in PA) and all(int(B.state[q]["step"]) == 3 for q in PB)
    want, gates = reference(before[0], grads, before[1], before[2], before[3], groups, MAX_NORM)
    ours, theirs = ((PA, A), (PB, B)) if ours_first else ((PB, B), (PA, A))
    for k, key in enumerate((None, "exp_avg", "exp_avg_sq")):
        for i in range(N_T):
            mine = get(ours[0][i] if key is None else ours[1].state[ours[0][i]][key]).astype(np.float64)
            other = get(theirs[0][i] if key is None else theirs[1].state[theirs[0][i]][key]).astype(np.float64)
            assert (np.abs(mine - want[k][i]) <= gates[k][i]).all(), (key, i)
            assert (np.abs(mine - other) <= gates[k][i]).all(), (key, i)
