"""Seed-trimmed graphs: the rows and edges each layer of an L-layer stack needs for the rows a script reads (csrc/hgt_trim.hip).

Every script of the reference reads the GNN's output at the seed rows only (`node_rep[x_ids]`, `node_rep[:len(ylabel)]`).  A row of
layer l's output matters only if it reaches a seed within the remaining L - l layers.  `np_trim_to_seeds` states once, in numpy, which
rows and edges that leaves and in which order they stand; `trim_to_seeds` builds the same arrays on the device:

  hop       hop[v] = length of the shortest directed path from v to any seed along source -> target edges (0 for a seed); -1 ("out")
            where it exceeds L = n_layers or no path exists.  EVERY edge counts, whatever its relation or its ends' types: a superset
            is harmless and keeps the rule independent of the schema.
  rows      kept iff 0 <= hop <= L, ordered by (hop, old row): order[i] = old row of new row i, new_id[v] = new row of v or -1.
  edges     kept iff hop[target] <= L - 1 (the source then has hop <= L), ordered by (hop[target], old position): edge_order[j] = old
            position of new edge j.
  counts    n_rows[k] = #{hop <= L - k}, k = 0..L (n_rows[L] = the distinct seeds); n_edges[l] = #{kept edges with hop[target] <= L - l},
            l = 1..L (n_edges[0] is set to n_edges[1] so that both tuples are indexed by the layer).  Both are non-increasing.
  layers    layer l (1-based) reads rows [0, n_rows[l-1]) and edges [0, n_edges[l]); its targets are rows [0, n_rows[l]); the adapter
            runs on rows [0, n_rows[0]).  Every target of layer l has ALL its in-edges inside that prefix, so its output is the
            untrimmed layer's output up to the rounding of another kernel route and row grouping.
  seeds     any order, repeats allowed; the stack's result is gathered at new_id[seeds] (`out_rows`).

A seed or an edge end outside [0, n_nodes) raises IndexError; n_layers outside [1, MAX_LAYERS] raises ValueError.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib

__all__ = ["np_trim_to_seeds", "np_trim_graph", "trim_to_seeds", "TrimmedGraph", "TrimArrays"]

MAX_LAYERS = _lib.HGT_TRIM_MAX_LAYERS
_MAX_N = 2 ** 31

TrimArrays = namedtuple("TrimArrays", "hop order new_id edge_order n_rows n_edges")


def _check_layers(n_layers):
    if int(n_layers) != n_layers or not 1 <= int(n_layers) <= MAX_LAYERS:
        raise ValueError("pyhgt_amd: n_layers must be in [1, %d], got %r" % (MAX_LAYERS, n_layers))
    return int(n_layers)


def np_trim_to_seeds(n_nodes, edge_index, seeds, n_layers):
    """The definition (module docstring).  edge_index [2, E]: row 0 the sources, row 1 the targets (the reference's wire format).
    -> TrimArrays(hop int32[N], order int64[n_rows[0]], new_id int64[N], edge_order int64[n_edges[1]], n_rows tuple[L + 1],
    n_edges tuple[L + 1])."""
    L = _check_layers(n_layers)
    N = int(n_nodes)
    if N < 0:
        raise ValueError("pyhgt_amd: n_nodes must not be negative")
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    ei = host(edge_index).astype(np.int64).reshape(2, -1)
    seeds = host(seeds).astype(np.int64).reshape(-1)
    src, dst = ei[0], ei[1]
    if seeds.size and (seeds.min() < 0 or seeds.max() >= N):
        raise IndexError("pyhgt_amd: a seed outside [0, n_nodes)")
    if src.size and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= N):
        raise IndexError("pyhgt_amd: edge_index contains node ids outside [0, n_nodes)")
    hop = np.full(N, -1, np.int32)
    hop[seeds] = 0
    for r in range(1, L + 1):                                   # level by level: the sources of the edges into the last level
        new = src[(hop[dst] == r - 1) & (hop[src] < 0)]
        hop[new] = r
    kept = np.flatnonzero(hop >= 0)
    order = kept[np.argsort(hop[kept], kind="stable")].astype(np.int64)
    new_id = np.full(N, -1, np.int64)
    new_id[order] = np.arange(order.size)
    ht = hop[dst]
    ekept = np.flatnonzero((ht >= 0) & (ht <= L - 1))
    edge_order = ekept[np.argsort(ht[ekept], kind="stable")].astype(np.int64)
    n_rows = tuple(int(np.count_nonzero((hop >= 0) & (hop <= L - k))) for k in range(L + 1))
    ne = [int(np.count_nonzero((ht >= 0) & (ht <= L - l))) for l in range(1, L + 1)]
    return TrimArrays(hop, order, new_id, edge_order, n_rows, tuple([ne[0]] + ne))


def np_trim_graph(trim, node_type, edge_index, edge_type, edge_time=None):
    """The renumbered, reordered graph tensors of a trim (int64): (node_type[order], new_id[edge_index[:, edge_order]],
    edge_type[edge_order], edge_time[edge_order] or None)."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    ei = host(edge_index).astype(np.int64).reshape(2, -1)
    eo = trim.edge_order
    return (host(node_type).astype(np.int64)[trim.order], trim.new_id[ei[:, eo]], host(edge_type).astype(np.int64)[eo],
            None if edge_time is None else host(edge_time).astype(np.int64)[eo])


# --------------------------------------------------------------------------------------------------------------- the device build
def _graph_tensors(graph, num_types, num_relations):
    if isinstance(graph, tuple) and len(graph) == 7:           # a _DeviceGraph / the 7-tuple of to_torch on the device
        _, node_type, edge_time, edge_index, edge_type, node_dict, edge_dict = graph
        num_types = len(node_dict) if num_types is None else num_types
        num_relations = len(edge_dict) if num_relations is None else num_relations
    elif len(graph) == 5:                                       # GNN.forward's arguments; the features are not looked at
        _, node_type, edge_time, edge_index, edge_type = graph
    elif len(graph) == 4:
        node_type, edge_time, edge_index, edge_type = graph
    else:
        raise ValueError("pyhgt_amd: trim_to_seeds takes a device graph or (node_type, edge_time, edge_index, edge_type)")
    return node_type, edge_time, edge_index, edge_type, num_types, num_relations


class TrimmedGraph:
    """Result of `trim_to_seeds`.  Device tensors: `.hop` int32[N]; `.order` int64[n_rows[0]]; `.new_id` int64[N]; `.edge_order`
    int64[n_edges[1]]; `.out_rows` int64[len(seeds)] = new_id[seeds]; the renumbered graph in the new order `.node_type`
    int64[n_rows[0]], `.edge_index` int64[2, n_edges[1]], `.edge_type`, `.edge_time` (None without times).  Host tuples `.n_rows`,
    `.n_edges` (indexed by the layer, 0..L), `.n_layers`, `.n_nodes`, `.n_seeds`.  `.plan(l, use_rte)` is the GraphPlan of layer l."""
    gathered = False       # True (NeighbourhoodGraph): the caller's node_feature already stands in the trim's row order

    def __init__(self):
        self._plans = {}
        self._i32 = {}

    def _as_int32(self, name):
        if name not in self._i32:
            self._i32[name] = getattr(self, name).to(torch.int32)
        return self._i32[name]

    @property
    def order32(self):
        """`.order` as int32, the index form hgt_gather_rows takes (made on first use, kept)."""
        return self._as_int32("order")

    @property
    def out_rows32(self):
        return self._as_int32("out_rows")

    def layer_graph(self, l):
        """(node_type, edge_index, edge_type, edge_time) of layer l (1-based): prefix views of the renumbered tensors."""
        if not 1 <= l <= self.n_layers:
            raise IndexError("layer %d of a trim for %d layers" % (l, self.n_layers))
        n, e = self.n_rows[l - 1], self.n_edges[l]
        return (self.node_type[:n], self.edge_index[:, :e], self.edge_type[:e], None if self.edge_time is None else self.edge_time[:e])

    def plan(self, l, use_rte=True):
        """The GraphPlan of layer l (1-based): rows [0, n_rows[l-1]), edges [0, n_edges[l]), targets [0, n_rows[l]).  Built on first
        use (hgt_plan_build: the hop-major node order is not type-contiguous) and kept with the trim."""
        from .conv import GraphPlan
        key = (int(l), bool(use_rte) and self.edge_time is not None)
        p = self._plans.get(key)
        if p is None:
            if self.num_types is None or self.num_relations is None:
                raise ValueError("pyhgt_amd: this trim was built without num_types / num_relations: it has no plans")
            nt, ei, et, tm = self.layer_graph(l)
            p = self._plans[key] = GraphPlan(nt, ei, et, tm if key[1] else None, self.num_types, self.num_relations, n_q_rows=self.n_rows[l])
        return p


def trim_to_seeds(graph, seeds, n_layers, num_types=None, num_relations=None):
    """(graph, seeds, n_layers) -> TrimmedGraph, built on the device: L + 8 launches whatever N and E, integer work only, every output
    equal to `np_trim_to_seeds` / `np_trim_graph` array for array.  graph: a device graph (`to_device_graph`, the device sampler,
    `stack_device_graphs`) or the tuple (node_type, edge_time, edge_index, edge_type) [with the features in front, as GNN.forward
    takes them] plus num_types / num_relations (needed for `.plan`).  seeds: int64 device tensor of rows, any order, repeats allowed.
    ONE host read: the 2 L + 1 counts and the bad-index flag, through pinned memory; no other synchronisation.
    IndexError: a seed or an edge end outside [0, n_nodes).  ValueError: n_layers outside [1, %d], N or E >= 2^31."""
    L = _check_layers(n_layers)
    node_type, edge_time, edge_index, edge_type, num_types, num_relations = _graph_tensors(graph, num_types, num_relations)
    if not node_type.is_cuda:
        raise RuntimeError("pyhgt_amd: trim_to_seeds builds on a GPU (no CPU fallback; the numpy definition is np_trim_to_seeds)")
    dev = node_type.device
    seeds = torch.as_tensor(seeds, device=dev)
    for name, t in (("node_type", node_type), ("edge_index", edge_index), ("edge_type", edge_type), ("seeds", seeds)) + (
            (("edge_time", edge_time),) if edge_time is not None else ()):
        if t.dtype != torch.int64:
            raise TypeError("pyhgt_amd: %s must be int64 like the reference's tensors, got %s" % (name, t.dtype))
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError("edge_index must be [2, E]")
    N, E, S = int(node_type.numel()), int(edge_index.size(1)), int(seeds.numel())
    if N >= _MAX_N or E >= _MAX_N or S >= _MAX_N:
        raise ValueError("pyhgt_amd: trim_to_seeds takes N, E and len(seeds) < 2^31")
    if edge_type.numel() != E or (edge_time is not None and edge_time.numel() != E):
        raise ValueError("edge_type / edge_time must have E entries")
    node_type, edge_type, seeds = node_type.contiguous(), edge_type.contiguous(), seeds.reshape(-1).contiguous()
    edge_time = None if edge_time is None else edge_time.contiguous()
    lib = _lib.load()
    need = C.c_uint64()
    _lib.check(lib.hgt_trim_tmp_bytes(N, E, L, C.byref(need)), "hgt_trim_tmp_bytes")
    i64 = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
    ptr = _lib.ptr
    sr, sc = (edge_index.stride(0), edge_index.stride(1)) if E > 0 else (0, 1)
    t = TrimmedGraph()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        tmp = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
        hop = torch.empty(N, dtype=torch.int32, device=dev)
        order, new_id, edge_order, ntype_out = i64(N), i64(N), i64(E), i64(N)
        ei_out, et_out, out_rows = i64(2, E), i64(E), i64(S)
        tm_out = None if edge_time is None else i64(E)
        counts = torch.empty(2 * L + 2, dtype=torch.int32, device=dev)
        host = _lib.pinned("trim_counts", 2 * MAX_LAYERS + 2, torch.int32)   # (the read waits for its event before the next trim starts)
        _lib.check(lib.hgt_trim_hops(ptr(edge_index), sr, sc, N, E, ptr(seeds), S, L, tmp.data_ptr(), tmp.numel(), stream.cuda_stream),
                   "hgt_trim_hops")
        _lib.check(lib.hgt_trim_fill(ptr(edge_index), sr, sc, ptr(edge_type), ptr(edge_time), ptr(node_type), N, E, ptr(seeds), S, L,
                                     tmp.data_ptr(), tmp.numel(), ptr(hop), ptr(order), ptr(new_id), ptr(edge_order), ptr(ntype_out),
                                     ptr(ei_out), ptr(et_out), ptr(tm_out), ptr(out_rows), counts.data_ptr(), host.data_ptr(),
                                     stream.cuda_stream), "hgt_trim_fill")
        tmp.record_stream(stream)
        done = torch.cuda.Event()
        done.record(stream)
        done.synchronize()                                       # the one host read of a trim
        c = host[:2 * L + 2].tolist()
    if c[2 * L + 1]:
        raise IndexError("pyhgt_amd: trim_to_seeds: a seed or an edge end outside [0, n_nodes)")
    t.n_layers, t.n_nodes, t.n_seeds = L, N, S
    t.num_types, t.num_relations = num_types, num_relations
    t.n_rows = tuple(c[:L + 1])
    t.n_edges = (c[L + 1],) + tuple(c[L + 1:2 * L + 1])
    n0, e1 = t.n_rows[0], t.n_edges[1]
    t.hop, t.new_id, t.out_rows = hop, new_id, out_rows
    t.order, t.edge_order, t.node_type = order[:n0], edge_order[:e1], ntype_out[:n0]
    t.edge_index, t.edge_type = ei_out[:, :e1], et_out[:e1]
    t.edge_time = None if tm_out is None else tm_out[:e1]
    return t


trim_to_seeds.__doc__ = trim_to_seeds.__doc__ % MAX_LAYERS
