"""Stacked batches, the part that needs no GPU: `merge_sampler_outputs` (the host sibling of `stack_device_graphs` and its oracle)
against a numpy restatement of the stacked node and edge order, the layout facts of tests/test_sampled.py on the merged batch, and
the C ABI additions.  The helpers here (the piece sets, the restatement) are shared with tests/test_stacked_batches_gpu.py.

The order (include/hgt_hip.h, hgt_stack_sorted):
  nodes   type, then piece, then the piece's own order
  edges   (sorted form) relation, then target type, then piece, then the piece's own order"""
import copy
import os
import re

import numpy as np
import pytest
import torch

from pyhgt_amd import _lib
from pyhgt_amd.sampled import merge_sampler_outputs, synthetic_sampled_batch, to_device_graph, to_torch_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE_SHAPES = [(8, 8, 2), (4, 16, 1), (16, 4, 3)]          # (n_seed, width, depth)


# ------------------------------------------------------------------ piece sets
def empty_type(batch, t):
    """The batch without any node of type t (and without the runs that touch it); the type keeps its (empty) self run."""
    feature, time, edge_list, graph = copy.deepcopy(batch)
    feature[t] = feature[t][:0]
    if time is not None:
        time[t] = time[t][:0]
    for tt in list(edge_list):
        for st in list(edge_list[tt]):
            if tt == t or st == t:
                del edge_list[tt][st]
    edge_list[t][t] = {"self": []}
    return feature, time, edge_list, graph


def without_relation(batch, rel):
    feature, time, edge_list, graph = copy.deepcopy(batch)
    hit = 0
    for tt in list(edge_list):
        for st in list(edge_list[tt]):
            if rel in edge_list[tt][st]:
                del edge_list[tt][st][rel]
                hit += 1
                if not edge_list[tt][st]:
                    del edge_list[tt][st]
    assert hit == 1, "the synthetic batch has no %s run" % rel
    return feature, time, edge_list, graph


def only_self(batch):
    feature, time, edge_list, graph = copy.deepcopy(batch)
    for tt in list(edge_list):
        for st in list(edge_list[tt]):
            if st != tt:
                del edge_list[tt][st]
            else:
                edge_list[tt][st] = {"self": edge_list[tt][st]["self"]}
    return feature, time, edge_list, graph


def piece_set(schema, feat_dim=16, seed=40):
    """Three pieces of different (n_seed, width, depth): the first has an empty type (the second type: an empty range in the middle
    of the ids), the second lacks a relation, the third has only `self` edges."""
    p = [synthetic_sampled_batch(schema, n_seed=s, width=w, depth=d, feat_dim=feat_dim, seed=seed + i)
         for i, (s, w, d) in enumerate(PIECE_SHAPES)]
    return [empty_type(p[0], "author"), without_relation(p[1], "PP_cite"), only_self(p[2])]


def tiny_pieces(n=33, feat_dim=8):
    """33 OAG pieces of 12 nodes: more pieces than half a wavefront, as many as the schema has relations (33)."""
    return [synthetic_sampled_batch("oag", n_seed=2, width=2, depth=1, feat_dim=feat_dim, seed=100 + i) for i in range(n)]


def without_time(pieces):
    return [(f, None, el, g) for f, _, el, g in pieces]


# ------------------------------------------------------------------ the order, restated with numpy (lexsort; the kernels search)
def restate_nodes(type_offs):
    """type_offs: per piece int array [T+1].  -> (stacked type_off [T+1], node_map [N_tot]: stacked row -> position in the
    piece-after-piece concatenation, new_id: per piece the stacked id of every local node)."""
    B, T = len(type_offs), len(type_offs[0]) - 1
    ntype = [np.repeat(np.arange(T), np.diff(o)) for o in type_offs]
    piece = np.concatenate([np.full(len(t), b) for b, t in enumerate(ntype)])
    local = np.concatenate([np.arange(len(t)) for t in ntype])
    node_map = np.lexsort((local, piece, np.concatenate(ntype)))          # last key first: type, piece, local
    inverse = np.empty_like(node_map)
    inverse[node_map] = np.arange(len(node_map))
    starts = np.concatenate([[0], np.cumsum([len(t) for t in ntype])])
    new_id = [inverse[starts[b]:starts[b + 1]] for b in range(B)]
    stacked_off = np.concatenate([[0], np.cumsum(np.bincount(np.concatenate(ntype), minlength=T))])
    return stacked_off, node_map, new_id


def restate_sorted(pieces_sorted):
    """pieces_sorted: per piece (src, dst, time or None, rel_ptr, type_off) as numpy arrays, ids local to the piece.
    -> dict of the stacked arrays and the two maps."""
    type_offs = [p[4] for p in pieces_sorted]
    T, R = len(type_offs[0]) - 1, len(pieces_sorted[0][3]) - 1
    stacked_off, node_map, new_id = restate_nodes(type_offs)
    src = np.concatenate([new_id[b][p[0]] for b, p in enumerate(pieces_sorted)]).astype(np.int64)
    dst = np.concatenate([new_id[b][p[1]] for b, p in enumerate(pieces_sorted)]).astype(np.int64)
    rel = np.concatenate([np.repeat(np.arange(R), np.diff(p[3])) for p in pieces_sorted])
    ttype = np.searchsorted(stacked_off, dst, side="right") - 1
    piece = np.concatenate([np.full(len(p[0]), b) for b, p in enumerate(pieces_sorted)])
    pos = np.concatenate([np.arange(len(p[0])) for p in pieces_sorted])
    edge_map = np.lexsort((pos, piece, ttype, rel))                       # relation, target type, piece, own order
    out = dict(src=src[edge_map], dst=dst[edge_map], rel_ptr=np.searchsorted(rel[edge_map], np.arange(R + 1)), type_off=stacked_off,
               node_map=node_map, edge_map=edge_map, time=None)
    if pieces_sorted[0][2] is not None:
        out["time"] = np.concatenate([p[2] for p in pieces_sorted])[edge_map]
    return out


def sorted_numpy(graph):
    return tuple(None if a is None else a.cpu().numpy() for a in graph.sorted)


def _nested_first_use(pieces):
    """Rank of every (target type, source type, relation) run in the merged edge_list: keys in the order the pieces first use them."""
    order = {}
    for _, _, el, _ in pieces:
        for tt in el:
            a = order.setdefault(tt, (len(order), {}))
            for st in el[tt]:
                b = a[1].setdefault(st, (len(a[1]), {}))
                for rel in el[tt][st]:
                    b[1].setdefault(rel, len(b[1]))
    return {(tt, st, rel): (a[0], b[0], c) for tt, a in order.items() for st, b in a[1].items() for rel, c in b[1].items()}


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("schema,T,R", [("mag", 4, 9), ("oag", 5, 33)])
def test_merged_batch_has_the_layout_of_the_reference_pipeline(schema, T, R):
    """The facts tests/test_sampled.py checks for one synthetic batch, on three merged pieces."""
    pieces = piece_set(schema)
    feature, time, edge_list, graph = merge_sampler_outputs(pieces)
    x, nt, tm, ei, et, node_dict, edge_dict = to_torch_layout(feature, time, edge_list, graph)
    assert len(graph.get_types()) == T and len(edge_dict) == R and edge_dict["self"] == R - 1
    assert x.size(0) == sum(len(f[t]) for f, _, _, _ in pieces for t in graph.get_types())
    assert torch.equal(nt, nt.sort().values)
    assert ei.shape[0] == 2 and ei.stride() == (1, 2)
    assert int(tm.min()) >= 111 and int(tm.max()) <= 129
    deg = torch.bincount(ei[1], minlength=nt.numel())
    assert int(deg.min()) >= 1                                                # every node has its self loop
    key = et * T + nt[ei[1]]
    starts = torch.cat([torch.tensor([0]), (key[1:] != key[:-1]).nonzero().flatten() + 1, torch.tensor([key.numel()])])
    seen_types = set()
    for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
        tgt = ei[1, a:b]
        assert torch.all(tgt[1:] >= tgt[:-1])
        t = int(nt[tgt[0]])
        if t not in seen_types:
            assert int(et[a]) == edge_dict["self"]
            seen_types.add(t)


@pytest.mark.parametrize("schema", ["mag", "oag"])
def test_merged_batch_is_the_pieces_relabelled(schema):
    """to_torch_layout(merged) == the pieces' to_torch_layout tensors with the node ids of the stacked order, the runs in the order
    the pieces first use them and the pieces one after the other inside a run; no edge joins two pieces."""
    pieces = piece_set(schema)
    types = pieces[0][3].get_types()
    x, nt, tm, ei, et, node_dict, edge_dict = to_torch_layout(*merge_sampler_outputs(pieces))
    lay = [to_torch_layout(*p) for p in pieces]
    type_offs = [np.array([l[5][t][0] for t in types] + [l[1].numel()]) for l in lay]
    assert any((np.diff(o) == 0).any() for o in type_offs), "one piece must have an empty type"
    assert len({tuple(np.unique(l[4].numpy())) for l in lay}) == 3, "the pieces must differ in the relations they use"
    assert set(np.unique(lay[2][4].numpy())) == {edge_dict["self"]}
    stacked_off, node_map, new_id = restate_nodes(type_offs)
    assert [node_dict[t] for t in types] == [[int(stacked_off[i]), i] for i in range(len(types))]
    assert torch.equal(x, torch.cat([l[0] for l in lay])[node_map])
    assert torch.equal(nt, torch.cat([l[1] for l in lay])[node_map])
    # edges: every piece's edge with its run's rank in the merged dictionary
    rank = _nested_first_use(pieces)
    rel_name = {v: k for k, v in edge_dict.items()}
    rows = []
    for b, l in enumerate(lay):
        src, dst, rel = l[3][0].numpy(), l[3][1].numpy(), l[4].numpy()
        tt, st = l[1].numpy()[dst], l[1].numpy()[src]
        for e in range(len(rel)):
            rows.append(rank[(types[tt[e]], types[st[e]], rel_name[rel[e]])] + (b, e, new_id[b][src[e]], new_id[b][dst[e]], rel[e],
                                                                                 int(l[2][e])))
    rows.sort()
    got = np.stack([ei[0].numpy(), ei[1].numpy(), et.numpy(), tm.numpy()], axis=1)
    assert np.array_equal(got, np.array([r[5:] for r in rows], dtype=np.int64))
    piece_of_row = np.searchsorted(np.cumsum([l[1].numel() for l in lay]), node_map, side="right")
    assert np.array_equal(piece_of_row[ei[0].numpy()], piece_of_row[ei[1].numpy()]), "an edge joins two pieces"
    assert np.array_equal(np.bincount(piece_of_row[ei[1].numpy()]), [l[4].numel() for l in lay])


@pytest.mark.parametrize("which", ["mag", "oag", "tiny33", "one", "mag-no-time"])
def test_sorted_form_of_the_merged_batch_is_the_stacked_order(which):
    """The int32 hand-off form (`.sorted`, built on the CPU with plan=False) of the merged batch == the restatement applied to the
    pieces' `.sorted` arrays: the equality the device path is tested with, here for its oracle."""
    pieces = {"mag": lambda: piece_set("mag"), "oag": lambda: piece_set("oag"), "tiny33": tiny_pieces,
              "one": lambda: piece_set("mag")[1:2], "mag-no-time": lambda: without_time(piece_set("mag"))}[which]()
    merged = to_device_graph(*merge_sampler_outputs(pieces), device="cpu", plan=False)
    assert merged.plan is None and merged.n_graphs == 1
    parts = [to_device_graph(*p, device="cpu", plan=False) for p in pieces]
    want = restate_sorted([sorted_numpy(g) for g in parts])
    got = sorted_numpy(merged)
    assert np.array_equal(got[0], want["src"]) and np.array_equal(got[1], want["dst"])
    assert (got[2] is None) == (want["time"] is None) == (which == "mag-no-time")
    if got[2] is not None:
        assert np.array_equal(got[2], want["time"])
    assert np.array_equal(got[3], want["rel_ptr"]) and np.array_equal(got[4], want["type_off"])
    assert got[0].dtype == np.int32 and got[3].dtype == np.int32
    assert sorted(want["edge_map"].tolist()) == list(range(len(got[0])))
    for a, b in zip(merged[:5], (torch.cat([g[0] for g in parts])[want["node_map"]], torch.cat([g[1] for g in parts])[want["node_map"]],
                                 None if got[2] is None else torch.cat([g[2] for g in parts])[want["edge_map"]], None,
                                 torch.cat([g[4] for g in parts])[want["edge_map"]])):
        if b is not None:
            assert torch.equal(a, b)
    if which == "one":
        for a, b in zip(sorted_numpy(parts[0]), got):
            assert np.array_equal(a, b)
        assert np.array_equal(want["node_map"], np.arange(len(want["node_map"])))


def test_to_device_graph_keeps_its_result_and_default():
    """plan=True stays the default and the 7-tuple is what it was; `.sorted` is additional."""
    import inspect
    sig = inspect.signature(to_device_graph)
    assert list(sig.parameters) == ["feature", "time", "edge_list", "graph", "device", "plan"] and sig.parameters["plan"].default is True
    g = to_device_graph(*piece_set("mag")[1], device="cpu", plan=False)
    assert isinstance(g, tuple) and len(g) == 7 and len(g.sorted) == 5
    ref = to_torch_layout(*piece_set("mag")[1])
    assert torch.equal(g[0], ref[0]) and torch.equal(g[1], ref[1]) and g[5] == ref[5] and g[6] == ref[6]
    assert torch.equal(g[3][0], g.sorted[0].long()) and torch.equal(g[3][1], g.sorted[1].long()) and torch.equal(g[2], g.sorted[2].long())


def test_merge_rejects_what_cannot_be_merged():
    mag, oag = piece_set("mag"), piece_set("oag")
    with pytest.raises(ValueError):
        merge_sampler_outputs([])
    with pytest.raises(ValueError):
        merge_sampler_outputs([mag[0], oag[0]])
    with pytest.raises(ValueError):
        merge_sampler_outputs([mag[1], synthetic_sampled_batch("mag", n_seed=4, width=4, depth=1, feat_dim=24, seed=1)])
    with pytest.raises(ValueError):
        merge_sampler_outputs([mag[1], without_time(mag)[2]])


def test_header_declares_the_stack_entry_points_under_abi_8():
    text = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+HGT_ABI_VERSION\s+8\b", code) and _lib.ABI_VERSION == 8
    assert int(re.search(r"#define\s+HGT_STACK_MAX_PIECES\s+(\d+)", code).group(1)) == _lib.HGT_STACK_MAX_PIECES
    ctype = {"int32_t": _lib._i32, "int64_t": _lib._i64, "uint64_t": _lib._u64}
    for name in ("hgt_stack_tmp_bytes", "hgt_stack_sorted"):
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert decl, "include/hgt_hip.h does not declare %s" % name
        params = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            base = p.rsplit(" ", 1)[0].replace("const ", "")
            if base.endswith("_host") or "_host" in p:      # host pointers: typed
                assert a is _lib.C.POINTER(ctype[base.rstrip("*").strip()]), (name, p)
            elif "*" in p:
                assert a is _lib._vp, (name, p)
            else:
                assert a is ctype[base], (name, p)
    # declared after the dropout block: appended, nothing moved
    assert code.index("hgt_stack_sorted") > code.index("hgt_dropout_apply")
    assert "hgt_stack.hip" in re.search(r"^SRCS\s*=\s*(.*?)(?<!\\)$", open(os.path.join(ROOT, "pyhgt_amd", "csrc", "Makefile")).read(),
                                        flags=re.M | re.S).group(1)


def test_library_exports_the_stack_entry_points():
    import ctypes as C
    lib = _lib.load()
    n = C.c_uint64()
    assert lib.hgt_stack_tmp_bytes(3, 4, 9, C.byref(n)) == 0 and n.value > 0 and n.value % 4 == 0
    assert lib.hgt_stack_tmp_bytes(0, 4, 9, C.byref(n)) == -1 and lib.hgt_stack_tmp_bytes(3, 4, 9, None) == -1
    assert lib.hgt_stack_tmp_bytes(_lib.HGT_STACK_MAX_PIECES + 1, 4, 9, C.byref(n)) == -2
    # bad arguments: a negative code before anything is launched (no device is touched: this runs on a machine without one)
    off = (C.c_int64 * 2)(0, 0)
    assert lib.hgt_stack_sorted(None, None, None, None, None, off, off, 1, 4, 9, None, None, None, None, None, None, None, None, 0, None) == -1
