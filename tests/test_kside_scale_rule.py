"""The scale rule of hgt_edge_logits_kside (csrc/hgt_edge_logits_kside.hip) without a GPU: the input sets that
tests/test_kside_logits_gpu.py feeds to the kernel, and the rule's quantisation alone, emulated in float64 on each of them.

The kernel brings K per (row, head) and A' = att_t per (relation, head) to a maximum in [2^14, 2^15) by an exact power of two
(kside_exp), splits both into fp16 hi + lo, sums hi hi + hi lo + lo hi (lo lo is dropped) and undoes the exponents at the end.  The
GPU tests bound the kernel's error by 2^-17 sum |q| |A'| |k| per (edge, head).  That bound has to hold for the NUMBER FORMAT before
it can say anything about the kernel: here the same products are summed exactly (float64), so what is left is the quantisation, and
it has to stay at or below half the bound on every input set -- uneven exponents per row and block, rows with a dominant half or
element, subnormal and huge rows.  The other half is for the kernel's ~130 fp32 roundings per logit."""
import math

import pytest
import torch

from oracle import hgt_oracle as O
from pyhgt_amd.synth import synthetic_typed_graph

DK = 32
BOUND = 2.0 ** -17
_cache = {}


# ------------------------------------------------------------------ input sets (CPU tensors, computed once, never modified)
def plain_inputs(N, E, H, T, R, seed, x_scale=1.0):
    """Q, K: the fp64 typed linears of x * x_scale rounded to fp32 (LayerNorm plays no part), att_t as hgt_relation_pack lays it out
    ([r][h][output j][k c] = relation_att[r][h][c][j] * pri / sqrt(d_k)), and a graph whose every 41st edge no relation claims."""
    key = ("plain", N, E, H, T, R, seed, x_scale)
    if key not in _cache:
        d = DK * H
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
        att_t = (sd["relation_att"].float().transpose(2, 3) * sd["relation_pri"].float().view(R, H, 1, 1) / math.sqrt(DK)).contiguous()
        _cache[key] = dict(N=N, E=E, d=d, H=H, T=T, R=R, sd=sd, nt=nt, ei=ei, et=et, Q=Q.float(), K=K.float(), att_t=att_t)
    return _cache[key]


UNEVEN = dict(N=300, E=270000, T=2, R=3)          # 64-edge work items: two or more batches per item, ragged tails
N_PAIR = 40                                       # edges written by hand between the rows of a special pair


def uneven_inputs(H):
    """plain_inputs with Q[n, h, :] * 2^a(n, h), K[n, h, :] * 2^b(n, h), a, b in [-40, 40], block (r, h) of att_t * 2^c(r, h), c in
    [-30, 30], drawn independently, and the special rows of `special` (name -> (what, node or relation, head)).  att_exp / zero_block
    are applied to att_t by edit_att (on the device: after hgt_relation_pack)."""
    key = ("uneven", H)
    if key in _cache:
        return _cache[key]
    p = plain_inputs(UNEVEN["N"], UNEVEN["E"], H, UNEVEN["T"], UNEVEN["R"], seed=40 + H)
    N, E, R = p["N"], p["E"], p["R"]
    g = torch.Generator().manual_seed(1000 + H)
    a = torch.randint(-40, 41, (N, H), generator=g)
    b = torch.randint(-40, 41, (N, H), generator=g)
    c = torch.randint(-30, 31, (R, H), generator=g)
    Q0, K0 = p["Q"].view(N, H, DK), p["K"].view(N, H, DK)
    Q = torch.ldexp(Q0, a.unsqueeze(-1)).contiguous()
    K = torch.ldexp(K0, b.unsqueeze(-1)).contiguous()
    sp = {}

    def head(i):
        return i % H
    # all-zero head rows
    sp["k_zero"] = ("K", 10, head(0))
    K[10, head(0)] = 0
    sp["q_zero"] = ("Q", 11, head(1))
    Q[11, head(1)] = 0
    # one half of the row 2^20 below the other: the scale is the maximum over BOTH halves of the row (two lanes hold one row)
    sp["k_low_half_small"] = ("K", 12, head(2))
    K[12, head(2), :16] *= 2.0 ** -20
    sp["k_high_half_small"] = ("K", 13, head(3))
    K[13, head(3), 16:] *= 2.0 ** -20
    sp["q_low_half_small"] = ("Q", 14, head(4))
    Q[14, head(4), :16] *= 2.0 ** -20
    sp["q_high_half_small"] = ("Q", 15, head(5))
    Q[15, head(5), 16:] *= 2.0 ** -20
    # a single element 2^20 above the rest
    sp["k_dominant"] = ("K", 16, head(6))
    K[16, head(6), 5] *= 2.0 ** 20
    sp["q_dominant"] = ("Q", 17, head(7))
    Q[17, head(7), 21] *= 2.0 ** 20
    # a K row of subnormals against a Q row at 2^60, a Q row at 2^120 against a K row at 2^-100 (absolute magnitudes: the rows
    # of the plain set, O(1), moved there).  The two targets take edges from their partner only: against a K row at 2^40 and a
    # block at 2^30 their logits would leave fp32's range, which is not what is tested here
    sp["k_subnormal"] = ("K", 18, head(0))
    K[18, head(0)] = torch.round(K0[18, head(0)] * 2.0 ** 14) * 2.0 ** -149
    sp["q_2p60"] = ("Q", 19, head(0))
    Q[19] = Q0[19]                                 # (the other heads of the four rows keep plain magnitudes, K: below)
    Q[19, head(0)] = Q0[19, head(0)] * 2.0 ** 60
    sp["q_2p120"] = ("Q", 20, head(1))
    Q[20] = Q0[20]
    Q[20, head(1)] = Q0[20, head(1)] * 2.0 ** 120
    sp["k_2m100"] = ("K", 21, head(1))
    K[21, head(1)] = K0[21, head(1)] * 2.0 ** -100
    ei, et = p["ei"].clone(), p["et"].clone()
    away = (ei[1] == 19) | (ei[1] == 20)
    ei[1, away] = 22
    pos = torch.arange(N_PAIR) * (41 * 150) + 3    # (3 and 4 modulo 41: the relations below claim them)
    assert int(pos.max()) + 1 < E
    ei[0, pos], ei[1, pos], et[pos] = 18, 19, torch.arange(N_PAIR) % R
    ei[0, pos + 1], ei[1, pos + 1], et[pos + 1] = 21, 20, torch.arange(N_PAIR) % R
    for hh in range(H):
        if hh != head(0):
            K[18, hh] = K0[18, hh]
        if hh != head(1):
            K[21, hh] = K0[21, hh]
    sp["zero_block"] = ("A", 1, head(3))
    out = dict(p, Q=Q.view(N, -1).contiguous(), K=K.view(N, -1).contiguous(), ei=ei.contiguous(), et=et, att_exp=c, zero_block=(1, head(3)),
               special=sp)
    out["att_t"] = edit_att(out, p["att_t"].clone())
    _cache[key] = out
    return out


def edit_att(inp, att_t):
    """The edits of an input set on att_t ([R][H][32][32], fp32, any device): exact powers of two per block, one block zero."""
    if "att_exp" in inp:
        att_t = torch.ldexp(att_t, inp["att_exp"].to(att_t.device).view(inp["R"], inp["H"], 1, 1))
        r, h = inp["zero_block"]
        att_t[r, h] = 0
    return att_t.contiguous()


def special_edge_counts(inp):
    """Claimed edges that meet each special row / block / pair of an uneven set."""
    src, dst, et, R = inp["ei"][0], inp["ei"][1], inp["et"], inp["R"]
    claimed = et < R
    n = {}
    for name, (what, idx, h) in inp["special"].items():
        m = (src == idx) if what == "K" else (dst == idx) if what == "Q" else (et == idx)
        n[name] = int((m & claimed).sum())
    n["pair_subnormal"] = int(((src == 18) & (dst == 19) & claimed).sum())
    n["pair_huge"] = int(((src == 21) & (dst == 20) & claimed).sum())
    return n


def zero_logit_mask(inp):
    """[E][H]: logits that are exactly 0 -- unclaimed edges, edges out of the zero K row / into the zero Q row (that head), edges
    through the zero block (that head)."""
    src, dst, et, R, H = inp["ei"][0], inp["ei"][1], inp["et"], inp["R"], inp["H"]
    z = (et >= R).unsqueeze(1).repeat(1, H)
    if "special" in inp:
        sp = inp["special"]
        z[:, sp["k_zero"][2]] |= src == sp["k_zero"][1]
        z[:, sp["q_zero"][2]] |= dst == sp["q_zero"][1]
        z[:, sp["zero_block"][2]] |= et == sp["zero_block"][1]
    return z


# ------------------------------------------------------------------ fp64 reference and the emulated rule
def logits_fp64(Q, K, att_t, ei, et, R, H, edges=None):
    """fp64 logits of fp32 inputs, and sum |q| |A'| |k| per (edge, head): the scale of their rounding errors.  On the device of Q;
    edges: a subset of edge ids (the result has their rows), default all."""
    dev = Q.device
    Qd, Kd = Q.double().view(-1, H, DK), K.double().view(-1, H, DK)
    A = att_t.to(dev).double().view(R, H, DK, DK)          # [r][h][output j][k c]
    ids = torch.arange(et.numel(), device=dev) if edges is None else edges.to(dev)
    src, dst, rel = ei[0].to(dev)[ids], ei[1].to(dev)[ids], et.to(dev)[ids]
    ref = torch.zeros(ids.numel(), H, dtype=torch.float64, device=dev)
    mag = torch.zeros_like(ref)
    for r in range(R):
        sel = (rel == r).nonzero().flatten()
        k, q = Kd[src[sel]].transpose(0, 1), Qd[dst[sel]].transpose(0, 1)          # [h][e][dk]
        ref[sel] = (torch.bmm(k, A[r].transpose(1, 2)) * q).sum(-1).T
        mag[sel] = (torch.bmm(k.abs(), A[r].abs().transpose(1, 2)) * q.abs()).sum(-1).T
    return ref, mag


def kside_exp(max_abs):
    """kside_exp of the kernel on a tensor of fp32 maxima: the biased exponent, clamped to [14, 254]."""
    return (max_abs.float().contiguous().view(torch.int32) >> 23).clamp(14, 254)


def _split_f16(v32):
    hi = v32.half()
    lo = (v32 - hi.float()).half()
    return hi.double(), lo.double()


def emulated_rule(Q, K, att_t, ei, et, R, H, edges):
    """The kernel's operands, summed exactly: K and A' scaled by 2^(141 - kside_exp) in fp32, fp16 hi + lo by casts, the three
    products it keeps, all sums in float64 -- and the exact logit and magnitude sum of the SAME scaled operands (the scales are
    uniform over a head's dot, so error / bound is what it is for the unscaled ones).  Returns (emulated, exact, magnitudes)."""
    Kv, A = K.view(-1, H, DK), att_t.view(R, H, DK, DK)
    ks = torch.ldexp(torch.ones((), dtype=torch.float64), 141 - kside_exp(Kv.abs().amax(-1)))             # [N][H]
    as_ = torch.ldexp(torch.ones((), dtype=torch.float64), 141 - kside_exp(A.abs().amax((-1, -2))))       # [R][H]
    Ks = (Kv.double() * ks.unsqueeze(-1)).float()           # (the kernel's fp32 product: exact unless it leaves fp32's range)
    As = (A.double() * as_.view(R, H, 1, 1)).float()
    assert bool(torch.isfinite(Ks).all()) and float(Ks.abs().max()) < 2.0 ** 15 and float(As.abs().max()) < 2.0 ** 15
    kh, kl = _split_f16(Ks)
    ah, al = _split_f16(As)
    Qd = Q.double().view(-1, H, DK)
    src, dst, rel = ei[0][edges], ei[1][edges], et[edges]
    emu = torch.zeros(edges.numel(), H, dtype=torch.float64)
    exact, mag = torch.zeros_like(emu), torch.zeros_like(emu)
    for r in range(R):
        sel = (rel == r).nonzero().flatten()
        q = Qd[dst[sel]].transpose(0, 1)
        KH, KL, KX = (t[src[sel]].transpose(0, 1) for t in (kh, kl, Ks.double()))
        AH, AL, AX = (t[r].transpose(1, 2) for t in (ah, al, As.double()))
        emu[sel] = ((torch.bmm(KH, AL) + torch.bmm(KL, AH) + torch.bmm(KH, AH)) * q).sum(-1).T
        exact[sel] = (torch.bmm(KX, AX) * q).sum(-1).T
        mag[sel] = (torch.bmm(KX.abs(), AX.abs()) * q.abs()).sum(-1).T
    return emu, exact, mag


def check_edges(inp, n_random=20000, seed=0):
    """A subset of the claimed edges: every edge that meets a special row of the set (at most 400 per row) and n_random others."""
    src, dst, et, R = inp["ei"][0], inp["ei"][1], inp["et"], inp["R"]
    g = torch.Generator().manual_seed(seed)
    claimed = (et < R).nonzero().flatten()
    pick = [claimed[torch.randperm(claimed.numel(), generator=g)[:n_random]]]
    for what, idx, _ in inp.get("special", {}).values():
        if what != "A":
            m = (((src == idx) if what == "K" else (dst == idx)) & (et < R)).nonzero().flatten()
            pick.append(m[:400])
    return torch.unique(torch.cat(pick))


def many_batches_inputs():
    return plain_inputs(2000, 2097152, 8, 2, 3, seed=77)          # 512-edge items: 16 batches per item


def far_rows_inputs():
    return plain_inputs(8192, 60000, 8, 2, 3, seed=91)            # the rows that the 2 GiB test spreads over 2 200 000


INPUT_SETS = {"uneven-h2": lambda: uneven_inputs(2), "uneven-h4": lambda: uneven_inputs(4), "uneven-h8": lambda: uneven_inputs(8),
              "many-batches": many_batches_inputs, "far-rows": far_rows_inputs,
              "x-2^20": lambda: plain_inputs(600, 150000, 8, 3, 4, seed=21, x_scale=2.0 ** 20),
              "x-2^-20": lambda: plain_inputs(600, 150000, 8, 3, 4, seed=21, x_scale=2.0 ** -20)}


@pytest.mark.parametrize("name", list(INPUT_SETS))
def test_quantisation_of_the_scale_rule_is_within_half_the_bound(name):
    inp = INPUT_SETS[name]()
    edges = check_edges(inp)
    emu, exact, mag = emulated_rule(inp["Q"], inp["K"], inp["att_t"], inp["ei"], inp["et"], inp["R"], inp["H"], edges)
    err = (emu - exact).abs()
    bound = BOUND * mag
    worst = (err / bound.clamp(min=1e-300)).max().item()
    print("\n%s: %d edges, worst quantisation error / bound %.4f" % (name, edges.numel(), worst))
    assert bool(torch.isfinite(emu).all())
    assert bool((err[mag == 0] == 0).all())
    assert bool((err <= 0.5 * bound).all()), worst
    if "special" in inp:
        n = special_edge_counts(inp)
        assert min(n.values()) >= 32, n


def test_uneven_inputs_are_what_they_claim():
    """Exponents spread per row and per block, the special rows in place, every one met by at least 32 claimed edges, and every
    fp64 logit inside fp32's range (the kernel's logits must then be finite)."""
    for H in (2, 4, 8):
        inp = uneven_inputs(H)
        N, R = inp["N"], inp["R"]
        Q, K, A = inp["Q"].view(N, H, DK), inp["K"].view(N, H, DK), inp["att_t"].view(R, H, DK, DK)
        ek = kside_exp(K.abs().amax(-1))
        assert int(ek.max()) - int(ek.min()) > 100 and len(torch.unique(ek)) > 50
        assert len(torch.unique(kside_exp(A.abs().amax((-1, -2))))) >= min(R * H, 5)
        sp = inp["special"]
        assert float(K[10, sp["k_zero"][2]].abs().max()) == 0 and float(Q[11, sp["q_zero"][2]].abs().max()) == 0
        assert float(A[1, sp["zero_block"][2]].abs().max()) == 0
        k12, k13 = K[12, sp["k_low_half_small"][2]].abs(), K[13, sp["k_high_half_small"][2]].abs()
        assert float(k12[:16].max()) * 2.0 ** 12 < float(k12[16:].max()) and float(k13[16:].max()) * 2.0 ** 12 < float(k13[:16].max())
        q14, q15 = Q[14, sp["q_low_half_small"][2]].abs(), Q[15, sp["q_high_half_small"][2]].abs()
        assert float(q14[:16].max()) * 2.0 ** 12 < float(q14[16:].max()) and float(q15[16:].max()) * 2.0 ** 12 < float(q15[:16].max())
        k18 = K[18, sp["k_subnormal"][2]].abs()
        assert 0 < float(k18.max()) < 2.0 ** -126 and int(kside_exp(k18.max())) == 14
        assert float(Q[20, sp["q_2p120"][2]].abs().max()) > 2.0 ** 118 and float(K[21, sp["k_2m100"][2]].abs().max()) < 2.0 ** -96
        n = special_edge_counts(inp)
        assert min(n.values()) >= 32, n
        ref, _ = logits_fp64(inp["Q"], inp["K"], inp["att_t"], inp["ei"], inp["et"], R, H, check_edges(inp, 60000))
        assert float(ref.abs().max()) < 2.0 ** 126
