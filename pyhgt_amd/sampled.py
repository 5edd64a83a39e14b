"""Device-side hand-off of sampled sub-graphs.

The reference turns a sampled batch into tensors with `to_torch(feature, time, edge_list, graph)`
(/root/reference/pyHGT/data.py:212-256): Python lists of int64 [source, target] pairs appended edge by edge, then
`LongTensor(...).t()`.  What the sampler hands it is already almost what the GPU plan needs:

  * node ids are type-contiguous, types ascending (data.py:227-235);
  * `edge_list[target_type][source_type][relation]` is a list of [target_serial, source_serial] pairs with the targets in
    ascending order inside every such run (data.py:199-209), the `self` run of a type first (data.py:183-186);
  * edge_time = year(target) - year(source) + 120 (data.py:250).

`to_device_graph` is a sibling of `to_torch` with the SAME inputs and the same 7-tuple result (the model code does not
change), but it (a) builds the arrays with numpy instead of per-edge list appends, (b) orders the runs relation-major --
inside one relation id the concatenated runs are then target-sorted, because a relation's runs belong to ascending target
types -- and (c) hands the int32 form of exactly that order to `hgt_plan_from_sorted`, which builds the GraphPlan without
the radix sorts of `hgt_plan_build`, and registers the plan for the tensors it returns: the first layer's
`GraphPlan.cached(...)` lookup hits.

Stacked batches: `stack_device_graphs` turns B such device graphs into ONE block-diagonal graph in the same sorted form on the
device (hgt_stack_sorted: three small launches, no sort, no host copy of an index), so that a loop which holds B sampled batches runs
them through the layers as one graph; `merge_sampler_outputs` is its host (numpy) sibling on sampler output.

`synthetic_sampled_batch` builds sampler OUTPUT (feature / time / edge_list dictionaries + a graph-like object) for the
ogbn-mag and OAG schemas -- the datasets themselves are not available offline -- with the layout facts above, for the
latency-regime benchmarks (BASELINE.json configs[2] and configs[4]) and the parity tests.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .conv import GraphPlan

__all__ = ["to_device_graph", "to_torch_layout", "synthetic_sampled_batch", "SchemaGraph", "MAG_META", "OAG_META",
           "merge_sampler_outputs", "stack_device_graphs"]

# (target_type, source_type, relation) triples in get_meta_graph() order; `rev_` twins as data.py:61 adds them
MAG_META = [("paper", "paper", "PP_cite"), ("paper", "paper", "rev_PP_cite"), ("paper", "author", "AP_write"),
            ("author", "paper", "rev_AP_write"), ("paper", "field_of_study", "PF_in"), ("field_of_study", "paper", "rev_PF_in"),
            ("author", "institution", "AI_in"), ("institution", "author", "rev_AI_in")]
_OAG_FWD = [("paper", "paper", "PP_cite"), ("paper", "field", "PF_in_L0"), ("paper", "field", "PF_in_L1"), ("paper", "field", "PF_in_L2"),
            ("paper", "field", "PF_in_L3"), ("paper", "field", "PF_in_L4"), ("paper", "field", "PF_in_L5"), ("paper", "venue", "PV_Conference"),
            ("paper", "venue", "PV_Journal"), ("paper", "venue", "PV_Repository"), ("paper", "venue", "PV_Patent"),
            ("paper", "author", "AP_write_first"), ("paper", "author", "AP_write_last"), ("paper", "author", "AP_write_other"),
            ("field", "field", "FF_in"), ("author", "affiliation", "in")]
OAG_META = _OAG_FWD + [(s, t, "rev_" + r) for (t, s, r) in _OAG_FWD]


class SchemaGraph:
    """The two methods of the reference's `Graph` that to_torch uses (data.py:72-83): get_types(), get_meta_graph()."""

    def __init__(self, types, meta):
        self._types, self._meta = list(types), list(meta)

    def get_types(self):
        return list(self._types)

    def get_meta_graph(self):
        return list(self._meta)


def synthetic_sampled_batch(schema="mag", n_seed=128, width=128, depth=6, feat_dim=None, mean_degree=6.0, seed=0):
    """Sampler-shaped output for a MAG-like (T=4, R=9 incl. `self`) or OAG-like (T=5, R=33) random graph:
    returns (feature, time, edge_list, graph) exactly as `sample_subgraph` would hand them to `to_torch`
    (data.py:86-210): per-type node budgets of n_seed + depth * width for the seed type and depth * width for the others,
    dict insertion order = seed type first, `self` run first, targets ascending inside a run, years in [2010, 2019]."""
    rng = np.random.default_rng(seed)
    if schema == "mag":
        types, meta, seed_type = ["paper", "author", "field_of_study", "institution"], MAG_META, "paper"
        feat_dim = feat_dim or 129
    elif schema == "oag":
        types, meta, seed_type = ["paper", "author", "field", "venue", "affiliation"], OAG_META, "paper"
        feat_dim = feat_dim or 1169
    else:
        raise ValueError("schema must be 'mag' or 'oag'")
    graph = SchemaGraph(types, meta)
    counts = {t: depth * width + (n_seed if t == seed_type else 0) for t in types}
    feature = {t: rng.standard_normal((counts[t], feat_dim)).astype(np.float32) for t in types}
    time = {t: rng.integers(2010, 2020, size=counts[t]) for t in types}
    order = [seed_type] + [t for t in types if t != seed_type]            # layer_data insertion order: seeds first
    edge_list = OrderedDict()
    for t in order:
        edge_list[t] = OrderedDict()
        edge_list[t][t] = OrderedDict()
        edge_list[t][t]["self"] = [[i, i] for i in range(counts[t])]      # data.py:183-186
    for (tt, st, rel) in meta:
        n_t, n_s = counts[tt], counts[st]
        deg = rng.poisson(mean_degree * n_s / max(1, sum(counts.values())) * len(types), size=n_t)
        deg = np.minimum(deg, n_s)
        pairs = []
        for ti in np.nonzero(deg)[0]:                                     # targets ascending (data.py:199-209)
            for si in rng.choice(n_s, size=deg[ti], replace=False):
                pairs.append([int(ti), int(si)])
        if pairs:
            edge_list[tt].setdefault(st, OrderedDict())[rel] = pairs
    return feature, time, edge_list, graph


def _runs(edge_list, node_off, edge_dict):
    """-> list of (relation id, target type offset, [n,2] int array of [target, source] GLOBAL ids) in dict order."""
    out = []
    for tt in edge_list:
        for st in edge_list[tt]:
            for rel in edge_list[tt][st]:
                pairs = np.asarray(edge_list[tt][st][rel], dtype=np.int64).reshape(-1, 2)
                if pairs.shape[0] == 0:
                    continue
                g = np.stack([pairs[:, 0] + node_off[tt], pairs[:, 1] + node_off[st]], axis=1)
                out.append((edge_dict[rel], node_off[tt], g))
    return out


def _feature_rows(mats):
    """Per-type feature arrays -> float32 [n, width] each; a type without nodes (any shape of size 0) takes the others' width."""
    mats = [np.asarray(a, dtype=np.float32) for a in mats]
    mats = [a if a.ndim == 2 else (a.reshape(len(a), -1) if a.size else np.zeros((0, 0), np.float32)) for a in mats]
    widths = sorted({a.shape[1] for a in mats if a.shape[0] > 0})
    if len(widths) > 1:
        raise ValueError("pyhgt_amd: feature arrays of different widths: %r" % (widths,))
    width = widths[0] if widths else max([a.shape[1] for a in mats] + [0])
    return [a if a.shape[0] > 0 else np.zeros((0, width), np.float32) for a in mats]


def _node_arrays(feature, time, graph):
    types = graph.get_types()
    node_dict, n = {}, 0
    for t in types:
        node_dict[t] = [n, len(node_dict)]
        n += len(feature[t])
    edge_dict = {e[2]: i for i, e in enumerate(graph.get_meta_graph())}
    edge_dict["self"] = len(edge_dict)
    feat = np.concatenate(_feature_rows([feature[t] for t in types]), axis=0)
    ntime = None if time is None else np.concatenate([np.asarray(time[t], dtype=np.int64).reshape(-1) for t in types])
    ntype = np.concatenate([np.full(len(feature[t]), node_dict[t][1], dtype=np.int64) for t in types])
    type_off = np.array([node_dict[t][0] for t in types] + [n], dtype=np.int32)
    return types, node_dict, edge_dict, feat, ntime, ntype, type_off


def to_torch_layout(feature, time, edge_list, graph):
    """The tensors `to_torch` returns (same order of nodes AND edges, data.py:212-256), built with numpy -- used to check
    that the synthetic batches and `to_device_graph` agree with the reference's wire format."""
    types, node_dict, edge_dict, feat, ntime, ntype, _ = _node_arrays(feature, time, graph)
    node_off = {t: node_dict[t][0] for t in types}
    runs = _runs(edge_list, node_off, edge_dict)
    tgt = np.concatenate([g[:, 0] for _, _, g in runs]) if runs else np.zeros(0, np.int64)
    src = np.concatenate([g[:, 1] for _, _, g in runs]) if runs else np.zeros(0, np.int64)
    et = np.concatenate([np.full(len(g), r, dtype=np.int64) for r, _, g in runs]) if runs else np.zeros(0, np.int64)
    etime = ntime[tgt] - ntime[src] + 120
    ei = torch.from_numpy(np.stack([src, tgt], axis=1)).t()                # [2, E] view with strides (1, 2), like data.py:254
    return (torch.from_numpy(feat), torch.from_numpy(ntype), torch.from_numpy(etime), ei, torch.from_numpy(et), node_dict, edge_dict)


def to_device_graph(feature, time, edge_list, graph, device="cuda", plan=True):
    """Sibling of `to_torch` (data.py:212-256): same arguments, same 7-tuple (node_feature, node_type, edge_time, edge_index,
    edge_type, node_dict, edge_dict) -- tensors already on `device` -- plus the GraphPlan, built from the sorted int32 form
    and registered for those tensors.  Edges are ordered relation-major (stable inside a relation); HGTConv's output does not
    depend on the edge order.  Returns the 7-tuple; the plan is `GraphPlan.cached(...)` away (or `.plan` of the result).

    The int32 arrays that are uploaded anyway stay with the result as `.sorted = (src32, dst32, time32, rel_ptr, type_off)`: what
    `stack_device_graphs` takes.  plan=False builds and registers no plan (`.plan` is None): for pieces that will only be stacked.
    time=None (layers without use_RTE) gives a graph without edge_time: element 2 of the tuple and of `.sorted` is None."""
    types, node_dict, edge_dict, feat, ntime, ntype, type_off = _node_arrays(feature, time, graph)
    node_off = {t: node_dict[t][0] for t in types}
    R = len(edge_dict)
    runs = _runs(edge_list, node_off, edge_dict)
    # relation-major; a relation's runs in ascending order of their target type offset -> targets non-decreasing per relation
    runs.sort(key=lambda r: (r[0], r[1]))
    if runs:
        tgt = np.concatenate([g[:, 0] for _, _, g in runs])
        src = np.concatenate([g[:, 1] for _, _, g in runs])
        rel = np.concatenate([np.full(len(g), r, dtype=np.int64) for r, _, g in runs])
    else:
        tgt = src = rel = np.zeros(0, np.int64)
    for r in range(R):      # the sampler guarantees ascending targets inside a run; verify once per relation (cheap, vectorised)
        seg = tgt[rel == r]
        if seg.size > 1 and np.any(seg[1:] < seg[:-1]):
            order = np.argsort(rel * (len(ntype) + 1) + tgt, kind="stable")   # generic fallback: one stable host sort
            tgt, src, rel = tgt[order], src[order], rel[order]
            break
    rel_ptr = np.searchsorted(rel, np.arange(R + 1)).astype(np.int32)
    dev = torch.device(device)
    node_feature = torch.from_numpy(feat).to(dev)
    node_type = torch.from_numpy(ntype).to(dev)
    # int32 form for the plan (12 B / edge over PCIe instead of 40 B of int64 wire format) ...
    src32 = torch.from_numpy(src.astype(np.int32)).to(dev)
    dst32 = torch.from_numpy(tgt.astype(np.int32)).to(dev)
    time32 = None if ntime is None else torch.from_numpy((ntime[tgt] - ntime[src] + 120).astype(np.int32)).to(dev)
    # ... and the reference's int64 tensors, derived on the device (forward() signature, keep_att order, backward plans)
    edge_index = torch.stack([src32.long(), dst32.long()], dim=1).t()
    edge_type = torch.repeat_interleave(torch.arange(R, device=dev), torch.from_numpy(np.diff(rel_ptr).astype(np.int64)).to(dev))
    edge_time = None if time32 is None else time32.long()
    T = len(types)
    rel_ptr_d, type_off_d = torch.from_numpy(rel_ptr).to(dev), torch.from_numpy(type_off).to(dev)
    out = _DeviceGraph((node_feature, node_type, edge_time, edge_index, edge_type, node_dict, edge_dict))
    out.sorted = (src32, dst32, time32, rel_ptr_d, type_off_d)
    if plan:
        out.plan = GraphPlan.from_sorted(node_type, edge_index, edge_type, edge_time, src32, dst32, time32, rel_ptr_d, type_off_d, T, R)
        GraphPlan.register(out.plan, node_type, edge_index, edge_type, edge_time, T, R)
    return out


class _DeviceGraph(tuple):
    """The 7-tuple of to_torch with the prebuilt plan attached (`.plan`) and the sorted int32 form it was built from (`.sorted`)."""
    plan = None
    sorted = None
    n_graphs = 1


# ------------------------------------------------------------------------------------------------ stacked batches
def _same_schema(what, a, b):
    if a != b:
        raise ValueError("pyhgt_amd: the batches disagree on %s: %r != %r" % (what, a, b))


def merge_sampler_outputs(batches):
    """B sampler outputs `(feature, time, edge_list, graph)` -> ONE tuple of the same shape that holds all of them as a graph without
    an edge between the pieces: per node type the feature / time arrays are concatenated piece after piece, and the serials in
    `edge_list[target_type][source_type][relation]` are shifted by the number of nodes of that type in the pieces before.  Inside
    one such run the pieces follow each other, so the targets stay ascending (data.py:199-209) and `to_torch` / `to_device_graph`
    take the result like any sampled batch.  Keys appear in the order in which the pieces first use them.  All batches must share
    the type list, the meta graph and the feature width; `time` may be None in all of them (or in none).  Host arrays only: the
    device path that avoids this merge and the second upload is `stack_device_graphs`."""
    batches = list(batches)
    if not batches:
        raise ValueError("pyhgt_amd: merge_sampler_outputs needs at least one batch")
    graph = batches[0][3]
    types, meta = list(graph.get_types()), [tuple(m) for m in graph.get_meta_graph()]
    for _, tm, _, g in batches:
        _same_schema("the node types", list(g.get_types()), types)
        _same_schema("the meta graph", [tuple(m) for m in g.get_meta_graph()], meta)
        if (tm is None) != (batches[0][1] is None):
            raise ValueError("pyhgt_amd: some batches carry node times and some do not")
    try:
        flat = _feature_rows([f[t] for f, _, _, _ in batches for t in types])
    except ValueError:
        raise ValueError("pyhgt_amd: the batches disagree on the feature width") from None
    feature = {t: np.concatenate(flat[i::len(types)], axis=0) for i, t in enumerate(types)}
    time = None if batches[0][1] is None else {t: np.concatenate([np.asarray(tm[t], dtype=np.int64).reshape(-1) for _, tm, _, _ in batches])
                                               for t in types}
    edge_list = OrderedDict()
    seen = {t: 0 for t in types}                     # nodes of a type in the pieces before
    for f, _, el, _ in batches:
        for tt in el:
            for st in el[tt]:
                for rel in el[tt][st]:
                    pairs = np.asarray(el[tt][st][rel], dtype=np.int64).reshape(-1, 2)
                    run = edge_list.setdefault(tt, OrderedDict()).setdefault(st, OrderedDict()).setdefault(rel, [])
                    run.append(pairs + np.array([seen[tt], seen[st]], dtype=np.int64))
        for t in types:
            seen[t] += len(f[t])
    for tt in edge_list:
        for st in edge_list[tt]:
            for rel in edge_list[tt][st]:
                edge_list[tt][st][rel] = np.concatenate(edge_list[tt][st][rel], axis=0)
    return feature, time, edge_list, graph


class _StackedGraph(_DeviceGraph):
    """Result of `stack_device_graphs`: the 7-tuple of the block-diagonal graph with `.plan`, `.sorted`, `.n_graphs`, the maps
    `.node_map` / `.edge_map` (stacked position -> position in the piece-after-piece concatenation, int32 on the device) and the
    two ways back to the pieces, `.rows` and `.unstack`."""
    node_map = None
    edge_map = None
    _types = None          # type names in id order
    _counts = None         # [piece][type id] -> number of nodes (host integers, from tensor shapes and node_dict)
    _node_off = None       # [piece] -> first position of the piece in the concatenation; entry B = number of nodes
    _inverse = None

    def rows(self, b, type_name, local_ids=None):
        """Stacked rows (int64 device tensor) of piece b's nodes of type `type_name`: all of them in the piece's order, or those with
        the given serials inside the type (a tensor or a sequence), e.g. `arange(n_seed)` for the seeds of a sampled batch."""
        t = self._types.index(type_name)
        if not 0 <= b < len(self._counts):
            raise IndexError("piece %d of a stack of %d" % (b, len(self._counts)))
        n = self._counts[b][t]
        base = self[5][type_name][0] + sum(self._counts[q][t] for q in range(b))
        dev = self[1].device
        if local_ids is None:
            return torch.arange(base, base + n, device=dev)
        return torch.as_tensor(local_ids, dtype=torch.int64, device=dev) + base

    def unstack(self, h):
        """[N, ...] tensor over the stacked nodes -> list of the B per-piece tensors [N_b, ...], each in its piece's own node order.
        Plain torch indexing: autograd flows through it."""
        if h.size(0) != self[1].numel():
            raise ValueError("unstack takes a tensor with one row per stacked node")
        if self._inverse is None:
            inv = torch.empty(self.node_map.numel(), dtype=torch.int64, device=self.node_map.device)
            inv[self.node_map.long()] = torch.arange(inv.numel(), device=inv.device)
            self._inverse = inv
        off = self._node_off
        return [h[self._inverse[off[b]:off[b + 1]]] for b in range(len(off) - 1)]


def stack_device_graphs(graphs):
    """B device graphs (results of `to_device_graph`, or of this function) -> one block-diagonal graph on the device: the
    `_DeviceGraph`-like 7-tuple (node_feature, node_type, edge_time, edge_index, edge_type, node_dict, edge_dict) that `GNN`,
    `HGTConv` and `Classifier` take like any other, with `.plan` built by `GraphPlan.from_sorted` and registered.

    Stacked node order: type, then piece, then the piece's own order; inside a relation the edges are ordered by target type, then
    piece, then the piece's own order -- the form `hgt_plan_from_sorted` needs, made by hgt_stack_sorted from the pieces' `.sorted`
    arrays without a sort.  The features are gathered once on the device (hgt_gather_rows through `.node_map`).  The layer computes
    per target and no edge joins two pieces, so the rows of the stacked output are the pieces' outputs (`.unstack`, `.rows`) up to
    the rounding of another kernel route, and the gradient of a loss summed over the pieces is the sum of the pieces' gradients.
    Dropout masks are drawn over the stacked rows: another draw than B separate steps'.

    No host synchronisation: every size comes from a tensor shape.  ValueError: an empty list, pieces that disagree on the node
    types, the relation dictionary, the feature width or on having edge_time, more than %d pieces (stack in two levels).  A piece
    whose `.sorted` arrays are not in the required form (targets not ascending inside a relation) is not detected here: the next
    forward raises the IndexError of `GraphPlan.raise_if_bad`, as it does for `GraphPlan.from_sorted`."""
    graphs = list(graphs)
    if not graphs:
        raise ValueError("pyhgt_amd: stack_device_graphs needs at least one graph")
    B = len(graphs)
    if B > _lib.HGT_STACK_MAX_PIECES:
        raise ValueError("pyhgt_amd: at most %d graphs per stack_device_graphs call, got %d (stack in two levels)"
                         % (_lib.HGT_STACK_MAX_PIECES, B))
    first = graphs[0]
    for g in graphs:
        if getattr(g, "sorted", None) is None:
            raise ValueError("pyhgt_amd: stack_device_graphs takes the results of to_device_graph / stack_device_graphs (no .sorted)")
    types = [k for k, _ in sorted(first[5].items(), key=lambda kv: kv[1][1])]
    T, R, dev, width = len(types), len(first[6]), first[0].device, first[0].size(1)
    has_time = first.sorted[2] is not None
    for g in graphs:
        _same_schema("the node types", [k for k, _ in sorted(g[5].items(), key=lambda kv: kv[1][1])], types)
        _same_schema("the node type ids", [g[5][k][1] for k in types], list(range(T)))
        _same_schema("the relation dictionary", dict(g[6]), dict(first[6]))
        _same_schema("the feature width", g[0].size(1), width)
        _same_schema("the device", g[0].device, dev)
        if g[0].dtype != torch.float32:
            raise TypeError("pyhgt_amd: node features must be float32")
        if (g.sorted[2] is not None) != has_time or (g[2] is not None) != has_time:
            raise ValueError("pyhgt_amd: some graphs carry edge_time and some do not")
    # host integers from tensor shapes and the node dictionaries
    n_nodes = [int(g[1].numel()) for g in graphs]
    n_edges = [int(g.sorted[0].numel()) for g in graphs]
    counts = []
    for g, n in zip(graphs, n_nodes):
        offs = [g[5][k][0] for k in types] + [n]
        counts.append([offs[t + 1] - offs[t] for t in range(T)])
    node_off = [0] + list(np.cumsum(n_nodes, dtype=np.int64))
    edge_off = [0] + list(np.cumsum(n_edges, dtype=np.int64))
    N, E = int(node_off[-1]), int(edge_off[-1])
    lib = _lib.load()
    tmp_bytes = C.c_uint64()
    _lib.check(lib.hgt_stack_tmp_bytes(B, T, R, C.byref(tmp_bytes)), "hgt_stack_tmp_bytes")
    src_c = torch.cat([g.sorted[0] for g in graphs])
    dst_c = torch.cat([g.sorted[1] for g in graphs])
    time_c = torch.cat([g.sorted[2] for g in graphs]) if has_time else None
    rel_ptr_c = torch.stack([g.sorted[3] for g in graphs]).contiguous()
    type_off_c = torch.stack([g.sorted[4] for g in graphs]).contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    src32, dst32, edge_map = torch.empty(E, **i32), torch.empty(E, **i32), torch.empty(E, **i32)
    time32 = torch.empty(E, **i32) if has_time else None
    rel_ptr, type_off, node_map = torch.empty(R + 1, **i32), torch.empty(T + 1, **i32), torch.empty(N, **i32)
    tmp = torch.empty(int(tmp_bytes.value), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(lib.hgt_stack_sorted(ptr(src_c), ptr(dst_c), ptr(time_c), ptr(rel_ptr_c), ptr(type_off_c),
                                        (C.c_int64 * (B + 1))(*[int(v) for v in edge_off]), (C.c_int64 * (B + 1))(*[int(v) for v in node_off]),
                                        B, T, R, ptr(src32), ptr(dst32), ptr(time32), ptr(rel_ptr), ptr(type_off), ptr(node_map),
                                        ptr(edge_map), ptr(tmp), tmp.numel(), stream.cuda_stream), "hgt_stack_sorted")
        tmp.record_stream(stream)
        # the features: one concatenation and one row gather through node_map, both on the device
        feat_c = torch.cat([g[0] for g in graphs]).contiguous()
        node_feature = torch.empty(N, width, dtype=torch.float32, device=dev)
        if N > 0 and width > 0:
            _lib.check(lib.hgt_gather_rows(feat_c.data_ptr(), width, node_map.data_ptr(), N, width, node_feature.data_ptr(),
                                           stream.cuda_stream), "hgt_gather_rows")
        feat_c.record_stream(stream)
        node_type = torch.cat([g[1] for g in graphs])[node_map.long()]
        edge_type = torch.cat([g[4] for g in graphs])[edge_map.long()]
        # the reference's int64 tensors, derived like to_device_graph derives them
        edge_index = torch.stack([src32.long(), dst32.long()], dim=1).t()
        edge_time = time32.long() if has_time else None
        node_dict, n = {}, 0
        for t, k in enumerate(types):
            node_dict[k] = [n, t]
            n += sum(c[t] for c in counts)
        out = _StackedGraph((node_feature, node_type, edge_time, edge_index, edge_type, node_dict, dict(first[6])))
        out.sorted = (src32, dst32, time32, rel_ptr, type_off)
        out.n_graphs, out.node_map, out.edge_map = B, node_map, edge_map
        out._types, out._counts, out._node_off = types, counts, [int(v) for v in node_off]
        out.plan = GraphPlan.from_sorted(node_type, edge_index, edge_type, edge_time, src32, dst32, time32, rel_ptr, type_off, T, R)
        GraphPlan.register(out.plan, node_type, edge_index, edge_type, edge_time, T, R)
    return out


stack_device_graphs.__doc__ = stack_device_graphs.__doc__ % _lib.HGT_STACK_MAX_PIECES
