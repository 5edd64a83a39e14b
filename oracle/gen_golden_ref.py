"""Generate tests/golden/ref/*.npz / *.json by running the REFERENCE's own modules (build container only).

TEST INFRASTRUCTURE.  The CPU tests that used to import the reference tree live compare against what it produced here, so
that they run on every machine:

  ref_to_torch.npz     pyHGT.data.to_torch on two small synthetic sampler batches (tests/test_sampled.py)
  ref_modules.json     state-dict names, shapes and repr of the reference's HGTConv / DenseHGTConv / GNN / Classifier /
                       Matcher (tests/test_capi.py)
  ref_live_conv.npz    one HGTConv forward (T=4 R=8 H=8 d=64, 1500 nodes / 12000 edges, RTE + LayerNorm) and the parameter
                       count of the published ogbn-mag model (tests/test_oracle.py)
  ref_backward_*.npz   gradients of <out, g> through the reference HGTConv / DenseHGTConv by torch.autograd (tests/test_oracle.py)
  ref_backward_dropout_*.npz   the same in training mode: the reference layer's nn.Dropout replaced by multiplication with
                       fixed masks (stored), so that oracle.backward_reference(drop_masks=...) is pinned to the reference's
                       own dropout sites (conv.py:125; DenseHGTConv conv.py:261 and conv.py:273)
  ref_gnn_pickle.npz   the bytes pickle.dumps writes for a reference GNN (its HGTConv has none of this project's runtime
                       attributes) and that GNN's state dict (tests/test_boundary.py)

Inputs and parameters are not stored where a seed rebuilds them (pyhgt_amd.synth / oracle.hgt_oracle.make_state_dict).

    python oracle/gen_golden_ref.py                       # rewrites the files above
    python oracle/gen_golden_ref.py --backward-dropout    # rewrites only ref_backward_dropout_*.npz
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
BACKWARD_DROPOUT = dict(T=3, R=4, H=4, d=32, N=300, E=2500, param_seed=24, graph_seed=25, g_seed=26, mask_seed=27, p=0.2)


def dropout_masks(case, dense):
    """The fixed dropout masks of the training-mode fixtures: (m1, m2) [N, d] of 0 or 1/(1-p) (m2 None for HGTConv)."""
    g = torch.Generator().manual_seed(case["mask_seed"] + int(dense))
    keep = 1.0 - case["p"]
    draw = lambda: torch.bernoulli(torch.full((case["N"], case["d"]), keep), generator=g) / keep
    m1 = draw()
    return m1, (draw() if dense else None)


class _FixedMaskDropout(torch.nn.Module):
    """Stands in for the reference layer's nn.Dropout: the k-th call multiplies by the k-th queued mask (the reference
    calls self.drop once per node type in HGTConv.update, twice per type in DenseHGTConv.update)."""

    def __init__(self, queue):
        super().__init__()
        self.queue = list(queue)

    def forward(self, x):
        m = self.queue.pop(0)
        assert m.shape == x.shape
        return x * m


def backward_dropout_fixtures(conv):
    """ref_backward_dropout_{hgt,dense}.npz: <out, g> and its gradients through the reference layer with fixed dropout masks."""
    b = BACKWARD_DROPOUT
    for dense in (False, True):
        sd = O.make_state_dict(b["d"], b["d"], b["T"], b["R"], b["H"], True, True, seed=b["param_seed"], dense=dense)
        x, nt, ei, et, tm = synthetic_typed_graph(b["N"], b["E"], b["d"], b["T"], b["R"], seed=b["graph_seed"])
        g = torch.randn(b["N"], b["d"], generator=torch.Generator().manual_seed(b["g_seed"]))
        m1, m2 = dropout_masks(b, dense)
        layer = (conv.DenseHGTConv if dense else conv.HGTConv)(b["d"], b["d"], b["T"], b["R"], b["H"], b["p"], True, True).eval()
        layer.load_state_dict(sd)
        queue = []
        for t in range(b["T"]):                      # the order of the reference's self.drop calls (conv.py:121-125 / 256-273)
            idx = nt == t
            if idx.sum() == 0:
                continue
            queue.append(m1[idx])
            if dense:
                queue.append(m2[idx])
        layer.drop = _FixedMaskDropout(queue)
        xr = x.clone().requires_grad_(True)
        out = layer(xr, nt, ei, et, tm)
        assert not layer.drop.queue, "the reference called its dropout fewer times than expected"
        (out * g).sum().backward()
        blob = {"x": xr.grad.numpy(), "out": out.detach().numpy(), "mask1": m1.numpy()}
        if dense:
            blob["mask2"] = m2.numpy()
        blob.update({"param::" + n: p.grad.numpy() for n, p in layer.named_parameters() if p.grad is not None})
        np.savez_compressed(os.path.join(GOLDEN, "ref_backward_dropout_%s.npz" % ("dense" if dense else "hgt")), **blob)


def module_record(m, with_repr=True):
    sd = m.state_dict()
    rec = {"keys": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()]}
    if with_repr:
        rec["repr"] = repr(m)
    return rec


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    os.makedirs(GOLDEN, exist_ok=True)
    if "--backward-dropout" in sys.argv:
        backward_dropout_fixtures(load_reference_conv())
        for name in ("ref_backward_dropout_hgt.npz", "ref_backward_dropout_dense.npz"):
            print(name, os.path.getsize(os.path.join(GOLDEN, name)), "bytes")
        return
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
    backward_dropout_fixtures(conv)
    # ---- a whole-module pickle written by the reference's classes
    torch.manual_seed(1)
    theirs = model.GNN(conv_name='hgt', in_dim=20, n_hid=32, n_heads=2, n_layers=2, dropout=0.2, num_types=2, num_relations=3)
    blob = pickle.dumps(theirs)
    np.savez_compressed(os.path.join(GOLDEN, "ref_gnn_pickle.npz"), blob=np.frombuffer(blob, dtype=np.uint8),
                        state_keys=np.array(json.dumps(list(theirs.state_dict().keys()))),
                        **{"param::" + k: v.numpy() for k, v in theirs.state_dict().items()})
    for name in ("ref_to_torch.npz", "ref_modules.json", "ref_live_conv.npz", "ref_backward_hgt.npz", "ref_backward_dense.npz",
                 "ref_backward_dropout_hgt.npz", "ref_backward_dropout_dense.npz", "ref_gnn_pickle.npz"):
        print(name, os.path.getsize(os.path.join(GOLDEN, name)), "bytes")


if __name__ == "__main__":
    main()
