"""CPU tests: the oracle against the reference's own outputs (golden fixtures, tests/golden/*.npz and
tests/golden/ref/: recorded from the reference executed live by oracle/gen_golden*.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import hgt_oracle as O
from oracle.gen_golden_ref import BACKWARD, BACKWARD_DROPOUT, LIVE_CONV, dropout_masks
from pyhgt_amd.synth import synthetic_typed_graph

REF_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref")

TOL = 1e-4   # BASELINE.json north_star: within 1e-4 fp32


def test_closed_form_matches_golden(golden):
    g = golden
    out, att = O.forward_closed_form(g["sd"], g["T"], g["R"], g["H"], g["x"], g["node_type"], g["edge_index"],
                                     g["edge_type"], g["edge_time"], use_norm=g["use_norm"], use_RTE=g["use_RTE"],
                                     dtype=torch.float64, return_att=True, dense=g["dense"])
    assert (out.float() - g["out"]).abs().max().item() < 2e-5
    assert (att.float() - g["att"]).abs().max().item() < 2e-6
    out32 = O.forward_closed_form(g["sd"], g["T"], g["R"], g["H"], g["x"], g["node_type"], g["edge_index"],
                                  g["edge_type"], g["edge_time"], use_norm=g["use_norm"], use_RTE=g["use_RTE"],
                                  dtype=torch.float32, dense=g["dense"])
    assert (out32 - g["out"]).abs().max().item() < 2e-5


def test_reference_cost_port_matches_golden(golden):
    g = golden
    if g["E"] > 10000:
        pytest.skip("port is the slow path; covered on the small fixtures")
    if g["dense"]:
        pytest.skip("the timed CPU port restates HGTConv (the benchmarked layer) only")
    out, att = O.forward_meta_relation_port(g["sd"], g["T"], g["R"], g["H"], g["x"], g["node_type"],
                                            g["edge_index"], g["edge_type"], g["edge_time"],
                                            use_norm=g["use_norm"], use_RTE=g["use_RTE"], return_att=True)
    assert (out - g["out"]).abs().max().item() < 2e-5
    assert (att - g["att"]).abs().max().item() < 2e-6


def test_attention_rows_sum_to_one(golden):
    g = golden
    _, att = O.forward_closed_form(g["sd"], g["T"], g["R"], g["H"], g["x"], g["node_type"], g["edge_index"],
                                   g["edge_type"], g["edge_time"], use_norm=g["use_norm"], use_RTE=g["use_RTE"],
                                   return_att=True, dense=g["dense"])
    dst = g["edge_index"][1]
    s = torch.zeros(g["N"], g["H"], dtype=att.dtype).index_add_(0, dst, att)
    has_in = torch.zeros(g["N"], dtype=torch.bool)
    has_in[dst] = True
    assert (s[has_in] - 1.0).abs().max().item() < 1e-9
    assert s[~has_in].abs().max().item() == 0.0 if (~has_in).any() else True


def test_edge_permutation_invariance():
    T, R, H, d = 3, 4, 4, 32
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=5)
    x, nt, ei, et, tm = synthetic_typed_graph(300, 2000, d, T, R, seed=6)
    a = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm)
    p = torch.randperm(2000, generator=torch.Generator().manual_seed(1))
    b = O.forward_closed_form(sd, T, R, H, x, nt, ei[:, p], et[p], tm[p])
    assert (a - b).abs().max().item() < 1e-10


def test_out_of_range_relation_is_zero_logit():
    """conv.py:68-69: edges no meta relation claims keep logit 0 / message 0 but stay in the softmax."""
    T, R, H, d = 2, 3, 2, 16
    sd = O.make_state_dict(d, d, T, R, H, True, False, seed=2)
    x, nt, ei, et, tm = synthetic_typed_graph(50, 300, d, T, R, seed=3)
    et2 = et.clone()
    et2[::7] = R + 1
    o_cf = O.forward_closed_form(sd, T, R, H, x, nt, ei, et2, None, use_RTE=False, dtype=torch.float32)
    o_pt = O.forward_meta_relation_port(sd, T, R, H, x, nt, ei, et2, None, use_RTE=False)
    assert (o_cf - o_pt).abs().max().item() < 2e-5


def test_live_reference_agrees_with_oracle_and_param_count():
    """Against one forward of the reference's own HGTConv (tests/golden/ref/ref_live_conv.npz, oracle/gen_golden_ref.py)."""
    z = np.load(os.path.join(REF_DIR, "ref_live_conv.npz"))
    c = LIVE_CONV
    T, R, H, d = c["T"], c["R"], c["H"], c["d"]
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=c["param_seed"])
    x, nt, ei, et, tm = synthetic_typed_graph(c["N"], c["E"], d, T, R, seed=c["graph_seed"])
    ref = torch.from_numpy(z["out"])
    got = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, dtype=torch.float32)
    assert (ref - got).abs().max().item() < 2e-5
    # structural known answer published by the reference (ogbn-mag/README.md:30), counted on the reference's GNN + Classifier
    assert int(z["n_params_published_model"][0]) == 21173389


@pytest.mark.parametrize("dense", [False, True])
def test_backward_oracle_matches_autograd_through_the_live_reference(dense):
    """Oracle for the (not yet built) backward pass, SURVEY 8f-2: gradients of <out, g> with respect to the input features
    and every parameter, from oracle.backward_reference, against torch.autograd through the verbatim reference layer
    (eval mode, fp64 vs the reference's fp32 -> 2e-4 relative; tests/golden/ref/ref_backward_*.npz, oracle/gen_golden_ref.py)."""
    z = np.load(os.path.join(REF_DIR, "ref_backward_%s.npz" % ("dense" if dense else "hgt")))
    b = BACKWARD
    T, R, H, d, N, E = b["T"], b["R"], b["H"], b["d"], b["N"], b["E"]
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=b["param_seed"], dense=dense)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=b["graph_seed"])
    g = torch.randn(N, d, generator=torch.Generator().manual_seed(b["g_seed"]))
    got = O.backward_reference(sd, T, R, H, x, nt, ei, et, tm, g, dense=dense)

    def close(a, b):
        return (a.double() - b.double()).abs().max().item() <= 2e-4 * max(1.0, b.abs().max().item())
    assert close(torch.from_numpy(z["x"]), got["x"])
    names = [k[len("param::"):] for k in z.files if k.startswith("param::")]
    assert len(names) == len(sd)                # every parameter of the reference layer had a gradient
    for name in names:
        assert close(torch.from_numpy(z["param::" + name]), got[name]), name


@pytest.mark.parametrize("dense", [False, True])
def test_dropout_masks_sit_where_the_reference_drops(dense):
    """Training mode: oracle.backward_reference(drop_masks=(m1, m2)) against autograd through the verbatim reference layer whose
    nn.Dropout was replaced by multiplication with the same fixed masks (tests/golden/ref/ref_backward_dropout_*.npz,
    oracle/gen_golden_ref.py) -- pins m1 to conv.py:125 (HGTConv) / conv.py:261 (DenseHGTConv) and m2 to conv.py:273."""
    z = np.load(os.path.join(REF_DIR, "ref_backward_dropout_%s.npz" % ("dense" if dense else "hgt")))
    b = BACKWARD_DROPOUT
    T, R, H, d, N, E = b["T"], b["R"], b["H"], b["d"], b["N"], b["E"]
    sd = O.make_state_dict(d, d, T, R, H, True, True, seed=b["param_seed"], dense=dense)
    x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, T, R, seed=b["graph_seed"])
    g = torch.randn(N, d, generator=torch.Generator().manual_seed(b["g_seed"]))
    m1, m2 = dropout_masks(b, dense)
    assert torch.equal(m1, torch.from_numpy(z["mask1"])) and (not dense or torch.equal(m2, torch.from_numpy(z["mask2"])))
    assert 0 < int((m1 == 0).sum()) < m1.numel()
    out = O.forward_closed_form(sd, T, R, H, x, nt, ei, et, tm, dense=dense, drop_masks=(m1, m2))
    assert (out - torch.from_numpy(z["out"]).double()).abs().max().item() < TOL
    got = O.backward_reference(sd, T, R, H, x, nt, ei, et, tm, g, dense=dense, drop_masks=(m1, m2))

    def close(a, b):
        return (a.double() - b.double()).abs().max().item() <= 2e-4 * max(1.0, b.abs().max().item())
    assert close(torch.from_numpy(z["x"]), got["x"])
    names = [k[len("param::"):] for k in z.files if k.startswith("param::")]
    assert len(names) == len(sd)
    for name in names:
        assert close(torch.from_numpy(z["param::" + name]), got[name]), name
    # the eval-mode oracle (no masks) is far from these numbers: the fixture really depends on where the masks sit
    assert not close(torch.from_numpy(z["x"]), O.backward_reference(sd, T, R, H, x, nt, ei, et, tm, g, dense=dense)["x"])
    if dense:                               # ... and swapping the two Dense masks is caught too
        swapped = O.backward_reference(sd, T, R, H, x, nt, ei, et, tm, g, dense=True, drop_masks=(m2, m1))
        assert not all(close(torch.from_numpy(z["param::" + n]), swapped[n]) for n in names)


@pytest.mark.parametrize("name", ["gnn_oag2", "gnn_mag4"])
def test_gnn_restatement_matches_reference_gnn_goldens(name):
    """oracle.gnn_forward (model.py:66-80 restated) against rows of every layer's output of the VERBATIM reference GNN
    (oracle/gen_golden_gnn.py: 2-layer OAG shape, published 4-layer n_hid=512 ogbn-mag model)."""
    import os
    import numpy as np
    from oracle.gen_golden_gnn import GNN_CASES, build_batch
    c = GNN_CASES[name]
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    _, (x, nt, tm, ei, et, _, _) = build_batch(c)
    assert x.size(0) == int(z["n_nodes"][0]) and et.numel() == int(z["n_edges"][0])
    sd = O.make_gnn_state_dict(c["in_dim"], c["n_hid"], c["T"], c["R"], c["H"], c["n_layers"], c["prev_norm"], c["last_norm"],
                               c["use_RTE"], seed=c["seed"])
    _, layers = O.gnn_forward(sd, c["in_dim"], c["n_hid"], c["T"], c["R"], c["H"], c["n_layers"], c["prev_norm"], c["last_norm"],
                              c["use_RTE"], x, nt, tm, ei, et, return_layers=True)
    rows = torch.from_numpy(z["rows"]).long()
    for i, h in enumerate(layers):
        err = (h[rows].float() - torch.from_numpy(z["layers"][i])).abs().max().item()
        assert err < 1e-5, (name, i, err)
