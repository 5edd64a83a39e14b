"""The CPU side of tests/test_degenerate_training_gpu.py: the fp64 oracle on every degenerate graph (forward and all gradients
finite), and the classification rule of that module (structural / cancelling / regular, computed from the graph) held against the
oracle's gradients -- which entries are exactly zero, which vanish by cancellation, and that every other slice is non-zero.  No GPU:
the module under test is imported for its graphs and its rule only."""
import pytest
import torch

import test_degenerate_training_gpu as DG

CASES = ([(name, 64, 4, dense) for name in DG.SQUARE for dense in (False, True)] + [(name, 64, 4, False) for name in DG.RECT] +
         [(name, d, H, False) for d, H, name in DG.LAYOUTS])


@pytest.mark.parametrize("name,d,H,dense", CASES, ids=["%s-d%d_h%d-%s" % (n, d, H, "dense" if de else "hgt") for n, d, H, de in CASES])
def test_the_rule_agrees_with_the_oracle(name, d, H, dense):
    g = DG.GRAPHS[name]
    sd, x, gout, fwd, ref = DG.reference(name, d, H, dense)
    assert bool(torch.isfinite(fwd).all())
    DG.check_rule_against_oracle(g, sd, ref)
    zero = sorted(k for k, r in ref.items() if not bool(r.any()))
    print("%s: %d of %d oracle gradients are identically zero" % (name, len(zero), len(ref)))


def test_the_graphs_have_the_properties_they_are_named_for():
    G, T, R = DG.GRAPHS, DG.T, DG.R
    assert G["no_edges"]["ei"].shape == (2, 0) and G["one_node_no_edge"]["nt"].numel() == 1
    assert G["single_edge"]["et"].tolist() == [R - 1] and G["single_edge"]["tm"].tolist() == [239]
    g = G["empty_type_isolated"]
    assert g["nt"].numel() == 63 and not bool((g["nt"] == 1).any()) and int(g["ei"][1].max()) < 20
    assert torch.unique(g["ei"][1]).numel() == 20                       # 43 targets without in-edges
    assert bool((G["all_unclaimed"]["et"] == R).all()) and bool((G["one_relation"]["et"] == 2).all())
    assert torch.equal(G["all_unclaimed"]["ei"], g["ei"]) and torch.equal(G["one_relation"]["ei"], g["ei"])
    g = G["ragged_65"]
    assert g["nt"].numel() == 65 and int(g["nt"][64]) == T + 1 and bool((g["ei"] == 64).any())
    for name in DG.RECT:
        g = G[name]
        assert g["NQ"] == 2 and g["nt"].numel() == 6 and int(g["ei"][1].max()) < 2 and not bool((g["ei"] == 5).any())
    # the cancelling kind occurs exactly where every target has one in-edge
    kinds = {name: {int(k) for key in ("q_linears.1.weight", "k_linears.0.weight", "k_linears.1.weight", "relation_att")
                    for k in DG.entry_kinds(G[name], key, (R, 4, 16, 16)).flatten()} for name in DG.SQUARE}
    assert [n for n in DG.SQUARE if DG.CANCELLING in kinds[n]] == ["one_node_self_loop", "single_edge"]


def test_the_gnn_rule_agrees_with_the_oracle():
    for name in ("empty_type_isolated", "no_edges"):
        g = DG.GRAPHS[name]
        sd, x, y, loss, ref = DG.gnn_reference(name, 37, 64, 4, 5)
        assert loss == loss
        for key, r in ref.items():
            assert bool(torch.isfinite(r).all()), key
            kinds = DG.gnn_entry_kinds(g, key, r.shape)
            assert not bool((kinds == DG.CANCELLING).any())
            assert bool((r[kinds.expand(r.shape) == DG.STRUCTURAL] == 0).all()), (name, key)
            if kinds.dim() == 0 and int(kinds) == DG.REGULAR:
                assert r.abs().max().item() > 0, (name, key)
