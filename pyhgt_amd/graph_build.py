"""The resident graph from raw edge lists, and the features of the types that have none (csrc/hgt_graph_build.hip).

The reference gets from OGB's `edge_index_dict` to its `Graph` with one Python step per edge (ogbn-mag/preprocess_ogbn_mag.py:29-42):

    for key in edge_index_dict:                      # key = (source type, relation, target type)
        elist = edg[t_type][s_type][r_type]
        rlist = edg[s_type][t_type]['rev_' + r_type]
        for s_id, t_id in edges.t().tolist():
            year = years[s_id] if s_type == 'paper' else years[t_id] if t_type == 'paper' else None
            elist[t_id][s_id] = year
            rlist[s_id][t_id] = year

`np_edge_lists_to_csr` states what that leaves behind -- and what `DeviceHeteroGraph.from_reference_graph` then reads out of it -- once,
in numpy; `DeviceHeteroGraph.from_edge_lists(device=...)` builds the same arrays on the device:

  triples   each key yields (target type, source type, relation): rows = the targets, neighbours = the sources; with `reverse` also
            (source type, target type, reverse + relation): rows = the sources, neighbours = the targets.
  order     inside a row the neighbours stand in the order of their FIRST appearance in the input (dict insertion order).
  repeats   a repeated (row, neighbour) pair keeps its first position and takes the LAST time given for it (the assignment overwrites).
  time      edge_time[key][e] if given, else node_time[source type][source id], else node_time[target type][target id], else none
            (TIME_NONE); `'paper'` of the script is "the types that have a node_time table".
  meta      the insertion order of the nested dicts, read as from_reference_graph reads them: target types by first appearance, under a
            target type its source types by first appearance, under those the relations.  The constructor's ordering of `triples` by
            (relation id, target type) applies on top, unchanged.
  degree    per type, a node's row lengths summed over the triples into its type -- after the repeats are gone (line 63).

Limits: 16 types and 48 triples, counted with the reverse relations; fewer than 2^31 - 1 edges per relation; a relation may not be
named `self` (from_reference_graph skips such a relation silently; here the caller chose the names), and two keys may not yield the same
triple (e.g. ('a', 'x', 'b') next to ('b', 'rev_x', 'a') with reverse='rev_').

`neighbour_mean` is lines 69-99 of the script -- normalize(coo(target, source)) . x -- as one gather-and-sum over the resident CSRs;
`np_neighbour_mean` is its definition in float64.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .sampler import TIME_NONE

__all__ = ["np_edge_lists_to_csr", "np_neighbour_mean", "neighbour_mean", "build_from_edge_lists"]

_TOO_LARGE = -4        # HGT_ERR_TOO_LARGE
_MAX_E = 2 ** 31 - 1


def _too_large(key, E):
    return RuntimeError("pyhgt_amd: relation %r: %d edges: N or E beyond 32-bit plan indices (code %d)" % (key, E, _TOO_LARGE))


def _plan(types, n_nodes, edges, edge_time, node_time, reverse):
    """The argument checks that need no edge data and the list of CSRs to build:
    -> (meta, jobs), jobs[i] = (key, forward?, time source) for meta[i]; time source = ('edge', key) | ('row' | 'nbr', type) | None."""
    types = list(types)
    if not 1 <= len(types) <= _lib.HGT_SAMPLER_MAX_TYPES:
        raise ValueError("pyhgt_amd: 1..%d node types, got %d" % (_lib.HGT_SAMPLER_MAX_TYPES, len(types)))
    edge_time, node_time = dict(edge_time or {}), dict(node_time or {})
    for t in types:
        if t not in n_nodes:
            raise ValueError("pyhgt_amd: n_nodes has no count for type %r" % (t,))
    for t in node_time:
        if t not in types:
            raise ValueError("pyhgt_amd: node_time for %r, which is not a node type" % (t,))
    for key in edge_time:
        if key not in edges:
            raise ValueError("pyhgt_amd: edge_time for %r, which is not a relation of `edges`" % (key,))
    nested, jobs = {}, {}
    for key in edges:
        if len(key) != 3:
            raise ValueError("pyhgt_amd: relation keys are (source type, relation, target type), got %r" % (key,))
        s_type, rel, t_type = key
        if s_type not in types or t_type not in types:
            raise ValueError("pyhgt_amd: relation %r joins types that are not node types" % (key,))
        if rel == "self" or (reverse is not None and reverse + rel == "self"):
            raise ValueError("pyhgt_amd: relation %r: the name `self` is taken by the self loops of every batch" % (key,))
        timed = key in edge_time
        if timed and (s_type in node_time or t_type in node_time):
            raise ValueError("pyhgt_amd: relation %r has both edge_time and a node_time table of one of its types" % (key,))
        by_src = s_type in node_time
        by_tgt = not by_src and t_type in node_time
        fwd = ("edge", key) if timed else ("nbr", s_type) if by_src else ("row", t_type) if by_tgt else None
        rev = ("edge", key) if timed else ("row", s_type) if by_src else ("nbr", t_type) if by_tgt else None
        for tri, job in [((t_type, s_type, rel), (key, True, fwd))] + ([] if reverse is None else [((s_type, t_type, reverse + rel), (key, False, rev))]):
            if tri in jobs:
                raise ValueError("pyhgt_amd: relation %r yields the meta triple %r a second time" % (key, tri))
            jobs[tri] = job
            nested.setdefault(tri[0], {}).setdefault(tri[1], []).append(tri[2])
    meta = [(tt, st, rel) for tt in nested for st in nested[tt] for rel in nested[tt][st]]
    if len(meta) > _lib.HGT_SAMPLER_MAX_TRIPLES:
        raise ValueError("pyhgt_amd: at most %d meta triples (reverse relations included), got %d" % (_lib.HGT_SAMPLER_MAX_TRIPLES, len(meta)))
    return meta, [jobs[tri] for tri in meta]


def _edge_shape(key, ei):
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError("pyhgt_amd: relation %r: edge_index must be [2, E], got %r" % (key, tuple(ei.shape)))
    E = int(ei.shape[1])
    if E >= _MAX_E:
        raise _too_large(key, E)
    return E


def _np_dict_csr(rows, nbrs, times, n_rows, n_nbrs):
    """the dict rule for one direction of one relation: entries (rows[e], nbrs[e], times[e]) in input order -> (indptr, nbr, time)"""
    E = rows.size
    key = rows * np.int64(max(n_nbrs, 1)) + nbrs
    order = np.argsort(key, kind="stable")                       # the copies of a pair side by side, in input order
    ks = key[order]
    edge = ks[1:] != ks[:-1]
    first = order[np.concatenate([[True], edge])] if E else order          # a pair's first entry: its position ...
    last = order[np.concatenate([edge, [True]])] if E else order           # ... and its last entry: its time
    by_row = np.lexsort((first, rows[first]))                     # rows ascending, inside a row by first appearance
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows[first], minlength=n_rows))]).astype(np.int32)
    return indptr, nbrs[first][by_row].astype(np.int32), times[last][by_row].astype(np.int32)


def np_edge_lists_to_csr(types, n_nodes, edges, edge_time=None, node_time=None, reverse="rev_"):
    """The definition (module docstring): -> (meta, csr) for DeviceHeteroGraph.from_csr, csr[i] = (indptr, src, time) of meta[i].
    Raises what from_edge_lists raises: ValueError for the arguments, IndexError for an id outside [0, n), the too-large error."""
    meta, jobs = _plan(types, n_nodes, edges, edge_time, node_time, reverse)
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    csr, ids = [None] * len(meta), {}
    for i in sorted(range(len(meta)), key=lambda i: list(edges).index(jobs[i][0])):       # relation by relation, as the script walks them
        (tt, st, _), (key, forward, tsrc) = meta[i], jobs[i]
        if key not in ids:
            ei = host(edges[key])
            E = _edge_shape(key, ei)
            if ei.dtype not in (np.int32, np.int64):
                raise ValueError("pyhgt_amd: relation %r: edge_index must be int32 or int64" % (key,))
            s, t = ei[0].astype(np.int64), ei[1].astype(np.int64)
            if E and (s.min() < 0 or s.max() >= n_nodes[key[0]] or t.min() < 0 or t.max() >= n_nodes[key[2]]):
                raise IndexError("pyhgt_amd: relation %r: a node id outside [0, n_nodes)" % (key,))
            ids = {key: (s, t)}
        s, t = ids[key]
        rows, nbrs = (t, s) if forward else (s, t)
        if tsrc is None:
            times = np.full(rows.size, TIME_NONE, np.int32)
        else:
            table = host(edge_time[key] if tsrc[0] == "edge" else node_time[tsrc[1]]).astype(np.int32).reshape(-1)
            want = rows.size if tsrc[0] == "edge" else n_nodes[tsrc[1]]
            if table.size != want:
                raise ValueError("pyhgt_amd: relation %r: the %s time table has %d entries, not %d" % (key, tsrc[0], table.size, want))
            times = table if tsrc[0] == "edge" else table[rows] if tsrc[0] == "row" else table[nbrs]
        csr[i] = _np_dict_csr(rows, nbrs, times, int(n_nodes[tt]), int(n_nodes[st]))
    return meta, csr


def _device_ids(key, a, device):
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        a = torch.from_numpy(a if all(s >= 0 for s in a.strides) else np.ascontiguousarray(a))
    _edge_shape(key, a)
    if a.dtype not in (torch.int32, torch.int64):
        raise ValueError("pyhgt_amd: relation %r: edge_index must be int32 or int64" % (key,))
    if a.device != device:                                  # upload as it lies in memory; a device tensor is read in place, strides and all
        a = a.to(device)
    return a


def _device_table(key, what, a, n, device):
    a = torch.as_tensor(a).reshape(-1)
    if a.numel() != n:
        raise ValueError("pyhgt_amd: relation %r: the %s time table has %d entries, not %d" % (key, what, a.numel(), n))
    return a.to(device=device, dtype=torch.int32).contiguous()


def build_from_edge_lists(cls, types, n_nodes, edges, edge_time=None, node_time=None, features=None, device=None, reverse="rev_"):
    """DeviceHeteroGraph.from_edge_lists.  device=None: the numpy definition and the ordinary constructor.  With a device: per input
    relation its one or two CSR builds are enqueued and their (kept entries, error flag) words are read in ONE host read; no edge array
    is copied to the host and no Python loop runs over edges or nodes."""
    types = list(types)
    if device is None:
        meta, csr = np_edge_lists_to_csr(types, n_nodes, edges, edge_time, node_time, reverse)
        return cls(types, meta, n_nodes, csr, features, None)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("pyhgt_amd: from_edge_lists builds on a GPU (no CPU fallback; device=None runs the numpy definition)")
    meta, jobs = _plan(types, n_nodes, edges, edge_time, node_time, reverse)
    edge_time, node_time = dict(edge_time or {}), dict(node_time or {})
    lib = _lib.load()
    by_key = {}
    for i, (key, _, _) in enumerate(jobs):
        by_key.setdefault(key, []).append(i)
    csr_dev = [None] * len(meta)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=device)
    tables = {}
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        for key, idx in by_key.items():
            ei = _device_ids(key, edges[key], device)
            E = int(ei.shape[1])
            if E and (int(n_nodes[key[0]]) < 1 or int(n_nodes[key[2]]) < 1):      # edges into a type without nodes: every id is outside
                raise IndexError("pyhgt_amd: relation %r: a node id outside [0, n_nodes)" % (key,))
            need = C.c_uint64()
            _lib.check(lib.hgt_graph_csr_bytes(E, C.byref(need)), "hgt_graph_csr_bytes(%r)" % (key,))
            ws = torch.empty(max(int(need.value), 256), dtype=torch.uint8, device=device)
            status = i32(2 * len(idx))
            built = []
            for j, i in enumerate(idx):
                tt, st, _ = meta[i]
                _, forward, tsrc = jobs[i]
                rows, nbrs = (ei[1], ei[0]) if forward else (ei[0], ei[1])
                et = nt = None
                if tsrc is not None and tsrc[0] == "edge":
                    if ("edge", key) not in tables:
                        tables[("edge", key)] = _device_table(key, "edge", edge_time[key], E, device)
                    et = tables[("edge", key)]
                elif tsrc is not None:
                    if ("node", tsrc[1]) not in tables:
                        tables[("node", tsrc[1])] = _device_table(key, "node", node_time[tsrc[1]], int(n_nodes[tsrc[1]]), device)
                    nt = tables[("node", tsrc[1])]
                by = _lib.HGT_GRAPH_TIME_BY_NBR if tsrc is not None and tsrc[0] == "nbr" else _lib.HGT_GRAPH_TIME_BY_ROW
                n_rows, n_nbrs = int(n_nodes[tt]), int(n_nodes[st])
                indptr, nbr_out, time_out = i32(n_rows + 1), i32(E), i32(E)
                ptr = _lib.ptr
                _lib.check(lib.hgt_graph_csr_build(ptr(rows), rows.stride(0), ptr(nbrs), nbrs.stride(0), rows.element_size(), ptr(et), ptr(nt),
                                                   by, E, n_rows, n_nbrs, indptr.data_ptr(), ptr(nbr_out), ptr(time_out),
                                                   status[2 * j:].data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream),
                           "hgt_graph_csr_build(%r)" % (key,))
                built.append((i, indptr, nbr_out, time_out))
            tables.pop(("edge", key), None)
            st_host = status.cpu().tolist()                  # the one host read of this relation: sizes and the error flag
            if any(st_host[2 * j + 1] for j in range(len(idx))):
                raise IndexError("pyhgt_amd: relation %r: a node id outside [0, n_nodes)" % (key,))
            for j, (i, indptr, nbr_out, time_out) in enumerate(built):
                kept = st_host[2 * j]
                if kept < E:                                  # repeats went: give the tail of the arrays back
                    nbr_out, time_out = nbr_out[:kept].clone(), time_out[:kept].clone()
                csr_dev[i] = (indptr, nbr_out, time_out)
    return cls._from_device_csr(types, meta, n_nodes, csr_dev, features, device)


# ------------------------------------------------------------------------------------------------------------------ neighbour mean
def _mean_triples(dgraph, target_type, source_type):
    if target_type not in dgraph.types or source_type not in dgraph.types:
        raise KeyError("pyhgt_amd: %r / %r are not node types of the graph" % (target_type, source_type))
    ms = [m for m, (tt, st, _) in enumerate(dgraph.triples) if tt == target_type and st == source_type]
    if not ms:
        raise KeyError("pyhgt_amd: no meta triple from %r into %r" % (source_type, target_type))
    return ms


def np_neighbour_mean(dgraph, target_type, source_type, x):
    """The definition in float64: out[r] = (sum of x[s] over the neighbours s of r) / their number, over all triples (target_type,
    source_type, *) in the order of dgraph.triples and a triple's neighbours in CSR order; a pair that two relations hold counts twice
    (coo_matrix sums it, preprocess_ogbn_mag.py:83); a row without neighbours is 0 (normalize's 1 / 0 -> 0, line 83)."""
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    n_rows = dgraph.n_nodes[dgraph.types.index(target_type)]
    total, count = np.zeros((n_rows, x.shape[1])), np.zeros(n_rows)
    for m in _mean_triples(dgraph, target_type, source_type):
        indptr, src, _ = dgraph.csr[m]
        rows = np.repeat(np.arange(n_rows), np.diff(indptr))
        np.add.at(total, rows, x[src])
        count += np.diff(indptr)
    return np.where(count[:, None] > 0, total / np.maximum(count, 1)[:, None], 0.0)


def neighbour_mean(dgraph, target_type, source_type, x, out=None):
    """Features of a type that has none, from those of its neighbours (preprocess_ogbn_mag.py:69-99): float32 [n_target, d], row r the
    mean of x's rows at r's neighbours of type source_type -- `np_neighbour_mean` in fp32, summed in the fixed order stated in
    include/hgt_hip.h (bit-reproducible, no float atomics).  x: float32 [n_source, d] on the graph's device with unit column stride; a
    column slice of a wider tensor is read in place.  out: likewise, [n_target, d].  One call on the current stream, no synchronisation."""
    if dgraph.device is None or dgraph.device.type != "cuda":
        raise RuntimeError("pyhgt_amd: neighbour_mean needs a DeviceHeteroGraph on a GPU (no CPU fallback; the host sibling is np_neighbour_mean)")
    ms = _mean_triples(dgraph, target_type, source_type)
    dev = dgraph.device
    n_rows, n_src = (dgraph.n_nodes[dgraph.types.index(t)] for t in (target_type, source_type))
    if not isinstance(x, torch.Tensor) or x.device != dev or x.dtype != torch.float32 or x.dim() != 2 or x.size(0) != n_src or x.size(1) < 1:
        raise ValueError("pyhgt_amd: x must be a float32 [%d, d >= 1] tensor on %s" % (n_src, dev))
    if x.size(0) and x.stride(1) != 1:
        x = x.contiguous()
    d = int(x.size(1))
    if out is None:
        out = torch.empty(n_rows, d, dtype=torch.float32, device=dev)
    elif (out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != (n_rows, d) or (n_rows and out.stride(1) != 1)
          or (n_rows > 1 and out.stride(0) < d)):
        raise ValueError("pyhgt_amd: out must be a float32 [%d, %d] tensor on %s with unit column stride" % (n_rows, d, dev))
    table = (_lib.HgtGraphCsr * len(ms))()
    n_entries = 0
    for j, m in enumerate(ms):
        ip, src, _ = dgraph.csr_dev[m]
        table[j] = _lib.HgtGraphCsr(ip.data_ptr(), src.data_ptr() if src.numel() else None)
        n_entries += int(src.numel())
    lib, need = _lib.load(), C.c_uint64()
    _lib.check(lib.hgt_neighbour_mean_bytes(n_entries, d, C.byref(need)), "hgt_neighbour_mean_bytes")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws = torch.empty(max(int(need.value), 256), dtype=torch.uint8, device=dev)
        ldx = max(int(x.stride(0)), d) if n_src > 1 else d
        ldo = max(int(out.stride(0)), d) if n_rows > 1 else d
        _lib.check(lib.hgt_neighbour_mean(table, len(ms), x.data_ptr() if x.numel() else None, ldx, n_rows, n_entries, d,
                                          out.data_ptr() if out.numel() else None, ldo, ws.data_ptr(), ws.numel(), stream.cuda_stream),
                   "hgt_neighbour_mean")
        ws.record_stream(stream)
    return out
