"""Generate tests/golden/ref/*.npz / *.json by running the REFERENCE's own modules (build container only).

TEST INFRASTRUCTURE.  The CPU tests that used to import the reference tree live compare against what it produced here, so
that they run on every machine:

  ref_to_torch.npz     pyHGT.data.to_torch on two small synthetic sampler batches (tests/test_sampled.py)
  ref_modules.json     state-dict names, shapes and repr of the reference's HGTConv / DenseHGTConv / GNN / Classifier /
                       Matcher (tests/test_capi.py)
  ref_live_conv.npz    one HGTConv forward (T=4 R=8 H=8 d=64, 1500 nodes / 12000 edges, RTE + LayerNorm) and the parameter
                       count of the published ogbn-mag model (tests/test_oracle.py)
  ref_backward_*.npz   gradients of <out, g> through the reference HGTConv / DenseHGTConv by torch.autograd (tests/test_oracle.py)
  ref_gnn_pickle.npz   the bytes pickle.dumps writes for a reference GNN (its HGTConv has none of this project's runtime
                       attributes) and that GNN's state dict (tests/test_boundary.py)

Inputs and parameters are not stored where a seed rebuilds them (pyhgt_amd.synth / oracle.hgt_oracle.make_state_dict).

    python oracle/gen_golden_ref.py        # rewrites the files above
"""
import json
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import hgt_oracle as O                                                           # noqa: E402
from oracle.reference_loader import load_reference_conv, load_reference_model, load_reference_data  # noqa: E402
from pyhgt_amd.sampled import synthetic_sampled_batch                                        # noqa: E402
from pyhgt_amd.synth import synthetic_typed_graph                                           # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ref")      # (a folder of its own: conftest.golden_names() globs tests/golden/*.npz)

# the cases, shared with the tests (the tests rebuild the inputs from these)
TO_TORCH_CASES = {"mag": dict(n_seed=16, width=12, depth=2, feat_dim=8, seed=3), "oag": dict(n_seed=16, width=12, depth=2, feat_dim=8, seed=3)}
LIVE_CONV = dict(T=4, R=8, H=8, d=64, N=1500, E=12000, param_seed=11, graph_seed=12)
BACKWARD = dict(T=3, R=4, H=4, d=32, N=300, E=2500, param_seed=21, graph_seed=22, g_seed=23)


def module_record(m, with_repr=True):
    sd = m.state_dict()
    rec = {"keys": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()]}
    if with_repr:
        rec["repr"] = repr(m)
    return rec


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    os.makedirs(GOLDEN, exist_ok=True)
    conv, model, data = load_reference_conv(), load_reference_model(), load_reference_data()
    # ---- to_torch
    blob = {}
    for schema, kw in TO_TORCH_CASES.items():
        ref = data.to_torch(*synthetic_sampled_batch(schema, **kw))
        for i, t in enumerate(ref[:5]):
            blob["%s/%d" % (schema, i)] = t.numpy()
        blob["%s/edge_index_stride" % schema] = np.array(ref[3].stride(), dtype=np.int64)
        blob["%s/dicts" % schema] = np.array(json.dumps([ref[5], ref[6]]))
    np.savez_compressed(os.path.join(GOLDEN, "ref_to_torch.npz"), **blob)
    # ---- module names / shapes / repr
    torch.manual_seed(0)
    mods = {"hgt_conv_norm_rte": module_record(conv.HGTConv(32, 32, 2, 3, 4, 0.2, True, True)),
            "hgt_conv_plain": module_record(conv.HGTConv(32, 32, 2, 3, 4, 0.2, False, False)),
            "dense_hgt_conv": module_record(conv.DenseHGTConv(32, 32, 2, 3, 4, 0.2, True, True)),
            "gnn": module_record(model.GNN(32, 64, 3, 4, 4, 2, prev_norm=True, last_norm=False, use_RTE=True)),
            "classifier": module_record(model.Classifier(32, 7)),
            "matcher": module_record(model.Matcher(32), with_repr=False)}      # (its __repr__ reads an attribute it never sets)
    with open(os.path.join(GOLDEN, "ref_modules.json"), "w") as f:
        json.dump(mods, f, indent=1)
    # ---- one live forward + the published model's parameter count
    c = LIVE_CONV
    sd = O.make_state_dict(c["d"], c["d"], c["T"], c["R"], c["H"], True, True, seed=c["param_seed"])
    layer = conv.HGTConv(c["d"], c["d"], c["T"], c["R"], c["H"], 0.2, True, True).eval()
    layer.load_state_dict(sd)
    x, nt, ei, et, tm = synthetic_typed_graph(c["N"], c["E"], c["d"], c["T"], c["R"], seed=c["graph_seed"])
    with torch.no_grad():
        out = layer(x, nt, ei, et, tm)
    net = torch.nn.Sequential(model.GNN(129, 512, 4, 9, 8, 4, prev_norm=True, last_norm=True, use_RTE=True), model.Classifier(512, 349))
    np.savez_compressed(os.path.join(GOLDEN, "ref_live_conv.npz"), out=out.numpy(),
                        n_params_published_model=np.array([sum(p.numel() for p in net.parameters())], dtype=np.int64))
    # ---- gradients through the reference layers
    b = BACKWARD
    for dense in (False, True):
        sd = O.make_state_dict(b["d"], b["d"], b["T"], b["R"], b["H"], True, True, seed=b["param_seed"], dense=dense)
        x, nt, ei, et, tm = synthetic_typed_graph(b["N"], b["E"], b["d"], b["T"], b["R"], seed=b["graph_seed"])
        g = torch.randn(b["N"], b["d"], generator=torch.Generator().manual_seed(b["g_seed"]))
        layer = (conv.DenseHGTConv if dense else conv.HGTConv)(b["d"], b["d"], b["T"], b["R"], b["H"], 0.2, True, True).eval()
        layer.load_state_dict(sd)
        xr = x.clone().requires_grad_(True)
        (layer(xr, nt, ei, et, tm) * g).sum().backward()
        grads = {"x": xr.grad.numpy()}
        grads.update({"param::" + n: p.grad.numpy() for n, p in layer.named_parameters() if p.grad is not None})
        np.savez_compressed(os.path.join(GOLDEN, "ref_backward_%s.npz" % ("dense" if dense else "hgt")), **grads)
    # ---- a whole-module pickle written by the reference's classes
    torch.manual_seed(1)
    theirs = model.GNN(conv_name='hgt', in_dim=20, n_hid=32, n_heads=2, n_layers=2, dropout=0.2, num_types=2, num_relations=3)
    blob = pickle.dumps(theirs)
    np.savez_compressed(os.path.join(GOLDEN, "ref_gnn_pickle.npz"), blob=np.frombuffer(blob, dtype=np.uint8),
                        state_keys=np.array(json.dumps(list(theirs.state_dict().keys()))),
                        **{"param::" + k: v.numpy() for k, v in theirs.state_dict().items()})
    for name in ("ref_to_torch.npz", "ref_modules.json", "ref_live_conv.npz", "ref_backward_hgt.npz", "ref_backward_dense.npz",
                 "ref_gnn_pickle.npz"):
        print(name, os.path.getsize(os.path.join(GOLDEN, name)), "bytes")


if __name__ == "__main__":
    main()
