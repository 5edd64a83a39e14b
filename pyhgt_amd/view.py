"""Whole-graph view of a resident graph (csrc/hgt_graph_view.hip): a `DeviceHeteroGraph` as the model's input, with no sampling.

The only way from a resident graph to `GNN.forward` used to be `sample_subgraph_device`.  `DeviceHeteroGraph.whole_graph` hands the
graph over as it is: the reference's wire format -- the 7-tuple of `to_torch` (pyHGT/data.py:212-256) -- for ALL nodes and all (or the
kept) edges, built on the device from the CSRs.  `np_whole_graph` states the rule once, in numpy:

  nodes      every node of every type; types in `dgraph.types` order, ids ascending inside a type: global row = type_off[type] + id,
             node_dict[t] = [type_off[t], index of t]; edge_dict = dgraph.edge_dict, `self` last (data.py:218-238).
  edges      the triples in the order of `dgraph.triples` (relation id, then target type), inside a triple in CSR order (row ascending,
             a row's neighbours in stored order): entry p of row r of (tt, st, rel) is the edge type_off[st] + src[p] -> type_off[tt] + r
             with edge_type = edge_dict[rel].  With self_loops the last run is one edge i -> i per node in row order, relation `self`
             (data.py:183-186); it is never filtered.  Inside one relation id the targets are non-decreasing: the form
             `hgt_plan_from_sorted` takes, so the plan needs no sort.
  node_time  {type: int array [n_type]} for every type that has nodes, or for none (anything else: ValueError).  Given: edge_time =
             node_time[target] - node_time[source] + 120 (data.py:250), 120 on a self loop; a value outside [0, 240) -- the
             reference's RTE table has 240 rows -- raises IndexError.  Absent: edge_time is None and the view serves layers with
             use_RTE=False only (the default of train_ogbn_mag.py).  WHICH time a node without a year of its own gets is the caller's
             decision: the reference defines it per sampled batch only (a sampled node inherits the time of the node it was reached
             from, data.py:125), so a whole graph has no such rule to copy.
  max_time   the sampler's rule (data.py:124-128): an entry with a stored time t is kept iff t <= max_time; an entry whose time is
             TIME_NONE takes node_time[target] under the same test when tables are given and is kept when there are none.  NODES are
             never dropped: a node newer than max_time keeps its row and its self loop, and the caller reads only the rows it means.
  leave_out  {(target type, source type, relation): (target_flags, source_flags)}, each None or a bool / uint8 array over that
             type's nodes: an entry is dropped iff target_flags[target] or source_flags[source] is set.  An unknown triple: KeyError.
             `label_edge_flags` builds the table of an evaluation whose labels are edges (train_paper_field.py:109-122).
  rel_ptr    rel_ptr[r] = the first kept position of relation id r; R + 1 entries, R = len(edge_dict).

What falls out, with no further code in the model: `gnn(*view[:5])[view.type_rows("paper")]` are the embeddings of all papers;
`gnn(*view[:5], seeds=view.rows("paper", ids))` is the exact L-layer output of those nodes (the seed trim works on any graph tensors);
the same calls under grad are full-batch training.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .conv import GraphPlan
from .sampled import _DeviceGraph
from .sampler import TIME_NONE, _host_array

__all__ = ["np_whole_graph", "label_edge_flags", "WholeGraphArrays", "VIEW_TILE"]

VIEW_TILE = _lib.HGT_VIEW_TILE          # entries one wavefront of the build takes; a workgroup takes 4 * VIEW_TILE
_MAX_E = 2 ** 31 - 1
_RTE_SELF = 120

WholeGraphArrays = namedtuple("WholeGraphArrays", "node_feature node_type edge_time edge_index edge_type node_dict edge_dict sorted")


# ------------------------------------------------------------------------------------------------------------ arguments
def _type_off(dgraph):
    return np.concatenate([[0], np.cumsum(dgraph.n_nodes)]).astype(np.int64)


def _node_dict(dgraph):
    off = _type_off(dgraph)
    return {t: [int(off[i]), i] for i, t in enumerate(dgraph.types)}


def _is_device(a):
    return isinstance(a, torch.Tensor) and a.is_cuda


def _node_time_tables(dgraph, node_time):
    """-> per type the caller's array (checked for its length; host values also for the int32 range), or None for no tables"""
    if not node_time:
        return None
    unknown = set(node_time) - set(dgraph.types)
    if unknown:
        raise KeyError("pyhgt_amd: node_time types %r are not node types of the graph" % sorted(unknown))
    out = []
    for t, n in zip(dgraph.types, dgraph.n_nodes):
        a = node_time.get(t)
        if a is None:
            if n > 0:
                raise ValueError("pyhgt_amd: node_time covers every type that has nodes or none of them; %r is missing" % t)
            out.append(np.zeros(0, np.int64))
            continue
        if not _is_device(a):
            a = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)
            if a.dtype.kind not in "iu":
                raise TypeError("pyhgt_amd: node_time[%r] must be an integer array" % t)
            a = a.astype(np.int64)
            if a.size and (a.min() <= TIME_NONE or a.max() >= 2 ** 31):
                raise ValueError("pyhgt_amd: node_time[%r] does not fit int32" % t)
        elif a.dtype not in (torch.int32, torch.int64):
            raise TypeError("pyhgt_amd: node_time[%r] must be an integer tensor" % t)
        elif a.dtype == torch.int64 and a.numel() and bool(((a <= TIME_NONE) | (a >= 2 ** 31)).any()):
            # (one host read; an int32 device table, the form the build takes, needs none)
            raise ValueError("pyhgt_amd: node_time[%r] does not fit int32" % t)
        if tuple(a.shape) != (n,):
            raise ValueError("pyhgt_amd: node_time[%r] must have one entry per node (%d), got shape %r" % (t, n, tuple(a.shape)))
        out.append(a)
    return out


def _leave_out_table(dgraph, leave_out):
    """-> per triple (target_flags, source_flags) in the order of dgraph.triples, each None or the caller's array (length checked);
    None for None / {}"""
    if not leave_out:
        return None
    where = {tri: m for m, tri in enumerate(dgraph.triples)}
    tid = {t: i for i, t in enumerate(dgraph.types)}
    table = [(None, None)] * len(dgraph.triples)
    for tri, pair in leave_out.items():
        tri = tuple(tri)
        if tri not in where:
            raise KeyError("pyhgt_amd: %r is not a meta triple of the graph" % (tri,))
        tf, sf = (f if f is None or isinstance(f, torch.Tensor) else np.asarray(f) for f in pair)
        for f, t in ((tf, tri[0]), (sf, tri[1])):
            if f is not None and tuple(f.shape) != (dgraph.n_nodes[tid[t]],):
                raise ValueError("pyhgt_amd: leave_out flags of %r over %r must have one entry per node" % (tri, t))
        table[where[tri]] = (tf, sf)
    return table


def _host_flags(f):
    return None if f is None else (f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)) != 0


def _flags_u8(f, dev):
    """a leave-out array (bool / uint8 / anything compared with 0) as a contiguous uint8 tensor on `dev`"""
    if not isinstance(f, torch.Tensor):
        f = torch.from_numpy(np.ascontiguousarray(np.asarray(f) != 0))
    elif f.dtype != torch.uint8:
        f = f != 0
    return f.to(device=dev, dtype=torch.uint8).contiguous()


def _feature_width(n_nodes, feats, types):
    """the common width of the feature matrices of the types that have nodes (ValueError: a type without one, differing widths); 0
    for a graph whose types are all empty"""
    widths = set()
    for t, n, f in zip(types, n_nodes, feats):
        if n == 0:
            continue
        if f is None:
            raise ValueError("pyhgt_amd: no feature matrix for node type %r" % t)
        widths.add(int(np.shape(f)[1]))
    if len(widths) > 1:
        raise ValueError("pyhgt_amd: feature matrices of different widths: %r" % (sorted(widths),))
    return widths.pop() if widths else 0


def _host_features(dgraph):
    """the types' feature matrices concatenated in type order (float32), or None for a graph that carries none"""
    feats = dgraph.features_host
    if feats is None:
        return None
    _feature_width(dgraph.n_nodes, feats, dgraph.types)
    mats = [_host_array(f) for n, f in zip(dgraph.n_nodes, feats) if n > 0]
    return np.concatenate(mats, axis=0) if mats else np.zeros((0, 0), np.float32)


def label_edge_flags(dgraph, relations, node_type, ids):
    """The `leave_out` table that takes the edges of `relations` at the nodes `ids` of `node_type` out of a whole-graph view, on both
    sides: for every meta triple whose relation is in `relations`, the target flags are set at `ids` if its target type is node_type
    and the source flags if its source type is.  label_edge_flags(dg, ["PF_in_L2", "rev_PF_in_L2"], "paper", test_ids) is the masking
    step of the reference's node_classification_sample (train_paper_field.py:109-122) for an evaluation whose labels are edges -- what
    `seed_edge_mask` is for a sampled batch, where the nodes are named by their serials.  Flags are uint8: device tensors on a device
    graph (ids may be a device tensor: nothing visits the host), numpy arrays on a host graph."""
    relations = set(relations)
    if node_type not in dgraph.types:
        raise KeyError("pyhgt_amd: %r is not a node type of the graph" % (node_type,))
    unknown = relations - {rel for _, _, rel in dgraph.triples}
    if unknown:
        raise KeyError("pyhgt_amd: %r are not relations of the graph" % sorted(unknown))
    n = dgraph.n_nodes[dgraph.types.index(node_type)]
    if _is_device(ids):                                  # no host read: an id outside [0, n) lands in a spare slot and names no node
        ids = ids.to(torch.int64).reshape(-1)
        flags = torch.zeros(n + 1, dtype=torch.uint8, device=ids.device)
        flags[torch.where((ids >= 0) & (ids < n), ids, torch.full_like(ids, n))] = 1
        flags = flags[:n].to(dgraph.device) if dgraph.device is not None else flags[:n].cpu().numpy()
    else:
        ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids, dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            raise IndexError("pyhgt_amd: ids of %r outside [0, %d)" % (node_type, n))
        flags = np.zeros(n, np.uint8)
        flags[ids] = 1
        if dgraph.device is not None:
            flags = torch.from_numpy(flags).to(dgraph.device)
    return {(tt, st, rel): (flags if tt == node_type else None, flags if st == node_type else None)
            for tt, st, rel in dgraph.triples if rel in relations}


# ------------------------------------------------------------------------------------------------------------ the definition
def _np_kept(time, rows, src, tgt_times, max_time, flags):
    """The entry rule (module docstring: max_time, leave_out) for entries of one triple: time[i] the stored time of entry i, rows[i] its
    target and src[i] its source (ids inside their types), tgt_times the node times of the target type or None for no tables,
    flags = (target_flags, source_flags) as `_leave_out_table` gives them, or None.  -> bool mask, True = kept.  The device statement
    is entry_kept (csrc/hgt_graph_rule.h)."""
    keep = np.ones(len(src), bool)
    if max_time is not None:
        t = np.asarray(time).astype(np.int64)
        none = t == TIME_NONE
        if tgt_times is not None:
            t = np.where(none, tgt_times[rows], t)
            none = np.zeros_like(none)
        keep &= none | (t <= int(max_time))
    if flags is not None:
        tf, sf = (_host_flags(f) for f in flags)
        if tf is not None:
            keep &= ~tf[rows]
        if sf is not None:
            keep &= ~sf[src]
    return keep


def _np_time_diff(tgt_times, src_times, rows, src, what):
    """edge_time of kept entries (module docstring: node_time) as int64; IndexError for a value outside [0, 240), with `what` = the
    caller and its triple in the message.  The device statement is entry_time_diff (csrc/hgt_graph_rule.h)."""
    dt = tgt_times[rows] - src_times[src] + _RTE_SELF
    if dt.size and (dt.min() < 0 or dt.max() >= _lib.HGT_RTE_LEN):
        raise IndexError("pyhgt_amd: %s outside [0, %d)" % (what, _lib.HGT_RTE_LEN))
    return dt


def np_whole_graph(dgraph, node_time=None, max_time=None, leave_out=None, self_loops=True):
    """The definition (module docstring) on `dgraph.csr`.  -> WholeGraphArrays: the numpy arrays of the 7-tuple (node_feature float32
    [N, width] or None for a graph without features, node_type int64[N], edge_time int64[E] or None, edge_index int64[2, E] with row 0
    the sources, edge_type int64[E], node_dict, edge_dict) and `.sorted` = (src32, dst32, time32 or None, rel_ptr int32[R + 1],
    type_off int32[T + 1]), the int32 form `to_device_graph` documents.

    ValueError: node_time covers some types with nodes but not all, or an array of the wrong length.  IndexError: a kept edge's
    time difference outside [0, 240).  KeyError: a `leave_out` triple the graph does not have.  Nodes are never dropped (max_time and
    leave_out filter edges only; the caller reads the rows it means), and which time a node without a year gets is the caller's
    decision (module docstring)."""
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    times = _node_time_tables(dgraph, node_time)
    if times is not None:
        times = [a.cpu().numpy().astype(np.int64) if isinstance(a, torch.Tensor) else a for a in times]
    table = _leave_out_table(dgraph, leave_out)
    type_off = _type_off(dgraph)
    N = int(type_off[-1])
    srcs, dsts, tms, per_rel = [], [], [], np.zeros(R, np.int64)
    for m, ((tt, st, rel), (indptr, src, time)) in enumerate(zip(dgraph.tri_types, dgraph.csr)):
        row = np.repeat(np.arange(dgraph.n_nodes[tt], dtype=np.int64), np.diff(indptr))
        s = src.astype(np.int64)
        keep = _np_kept(time, row, s, None if times is None else times[tt], max_time, None if table is None else table[m])
        row, s = row[keep], s[keep]
        srcs.append(s + type_off[st])
        dsts.append(row + type_off[tt])
        if times is not None:
            tms.append(_np_time_diff(times[tt], times[st], row, s, "whole_graph: a time difference of %r" % (dgraph.triples[m],)))
        per_rel[rel] += row.size
    if self_loops:
        srcs.append(np.arange(N, dtype=np.int64)); dsts.append(np.arange(N, dtype=np.int64))
        tms.append(np.full(N, _RTE_SELF, np.int64))
        per_rel[R - 1] += N
    cat = lambda a: np.concatenate(a).astype(np.int64) if a else np.zeros(0, np.int64)
    src, dst = cat(srcs), cat(dsts)
    if src.size >= _MAX_E:
        raise ValueError("pyhgt_amd: whole_graph takes fewer than 2^31 - 1 edges")
    etime = cat(tms) if times is not None else None
    rel_ptr = np.concatenate([[0], np.cumsum(per_rel)])
    node_type = np.repeat(np.arange(T, dtype=np.int64), dgraph.n_nodes)
    edge_type = np.repeat(np.arange(R, dtype=np.int64), per_rel)
    sorted_ = (src.astype(np.int32), dst.astype(np.int32), None if etime is None else etime.astype(np.int32),
               rel_ptr.astype(np.int32), type_off.astype(np.int32))
    return WholeGraphArrays(_host_features(dgraph), node_type, etime, np.stack([src, dst]), edge_type, _node_dict(dgraph),
                            dict(dgraph.edge_dict), sorted_)


# ------------------------------------------------------------------------------------------------------------ the view
class _Rows:
    """what a whole-graph view knows about its rows"""
    _n_nodes = None        # {type: count}

    def type_rows(self, type_name):
        """the global rows of a type as a slice: `rep[view.type_rows("paper")]`"""
        first = self[5][type_name][0]
        return slice(first, first + self._n_nodes[type_name])

    def rows(self, type_name, ids=None):
        """the global rows (int64 tensor on the view's device) of a type -- all of them, or those of the given ids of it (a tensor
        or a sequence; any order, repeats allowed): the `seeds=` of an exact inference"""
        first, dev = self[5][type_name][0], self[1].device
        if ids is None:
            return torch.arange(first, first + self._n_nodes[type_name], dtype=torch.int64, device=dev)
        return torch.as_tensor(ids, device=dev).to(torch.int64).reshape(-1) + first


class _HostWholeGraph(_Rows, tuple):
    """`whole_graph` of a host-only graph: the definition's 7-tuple as CPU tensors, `.sorted` as numpy arrays, no plan"""
    sorted = None
    plan = None


class _WholeDeviceGraph(_Rows, _DeviceGraph):
    """Result of `DeviceHeteroGraph.whole_graph` on a device graph: a `_DeviceGraph` (the 7-tuple with `.sorted` and `.plan`) with
    `.rows`, `.type_rows` and `.raise_if_bad`."""
    _head = None           # device int32[R + 2]: rel_ptr, then the build's flag word
    _bad = None            # the flag word once it has been read
    filtered = False

    def raise_if_bad(self, wait=False):
        """IndexError if a time difference is outside [0, 240).  A filtered view has checked before it returned.  An unfiltered one is
        built without a host read and copies nothing to the host: edge_time carries such a value as it is, so its plan flags the
        same edges in its header, and this call asks the plan (`GraphPlan.raise_if_bad(wait)`) -- as every layer's forward does,
        which is why the model does not depend on this call.  A view built with plan=False reads its own flag word from the device
        when wait=True (one host read) and knows nothing before."""
        if self.plan is not None:
            self.plan.raise_if_bad(wait=wait)
        if self._bad is None and wait:
            self._bad = int(self._head[-1])
        if (self._bad or 0) & _lib.HGT_VIEW_BAD_TIME:
            raise IndexError("pyhgt_amd: whole_graph: a time difference outside [0, %d)" % _lib.HGT_RTE_LEN)


def _host_view(dgraph, node_time, max_time, leave_out, self_loops):
    a = np_whole_graph(dgraph, node_time, max_time, leave_out, self_loops)
    if a.node_feature is None and a.node_type.size:
        raise ValueError("pyhgt_amd: the DeviceHeteroGraph carries no features")
    feat = np.zeros((0, 0), np.float32) if a.node_feature is None else a.node_feature
    tt = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x))
    out = _HostWholeGraph((tt(feat), tt(a.node_type), tt(a.edge_time), tt(a.edge_index), tt(a.edge_type), a.node_dict, a.edge_dict))
    out.sorted = a.sorted
    out._n_nodes = dict(zip(dgraph.types, dgraph.n_nodes))
    return out


def _device_features(dgraph):
    feats = dgraph.features
    if feats is None:
        raise ValueError("pyhgt_amd: the DeviceHeteroGraph carries no features")
    _feature_width(dgraph.n_nodes, feats, dgraph.types)
    mats = [f for n, f in zip(dgraph.n_nodes, feats) if n > 0]
    if not mats:
        return torch.zeros(0, 0, dtype=torch.float32, device=dgraph.device)
    return mats[0] if len(mats) == 1 else torch.cat(mats, dim=0)


def whole_graph(dgraph, node_time=None, max_time=None, leave_out=None, self_loops=True, plan=True):
    """`DeviceHeteroGraph.whole_graph` (its docstring has the interface; the module docstring the rule)."""
    if dgraph.device is None:
        return _host_view(dgraph, node_time, max_time, leave_out, self_loops)
    if dgraph.device.type != "cuda":
        raise RuntimeError("pyhgt_amd: whole_graph builds on a GPU (no CPU fallback; a host-only graph gets the numpy definition)")
    dev = dgraph.device
    T, R, M = len(dgraph.types), len(dgraph.edge_dict), len(dgraph.triples)
    times = _node_time_tables(dgraph, node_time)
    table = _leave_out_table(dgraph, leave_out)
    filtered = max_time is not None or table is not None
    node_feature = _device_features(dgraph)
    type_off = _type_off(dgraph)
    N = int(type_off[-1])
    n_csr = [int(c[1].numel()) for c in dgraph.csr_dev]              # sizes from tensor shapes: no host read
    first = np.concatenate([[0], np.cumsum(n_csr)]).astype(np.int64)
    E_cap = int(first[-1]) + (N if self_loops else 0)
    if E_cap >= _MAX_E:
        raise ValueError("pyhgt_amd: whole_graph takes fewer than 2^31 - 1 edges")
    keep_alive = []

    def dev_array(a, dtype):
        """a caller's array as a contiguous device tensor of `dtype`, its address (None for an empty one)"""
        if a is None:
            return None
        t = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dtype).contiguous()
        keep_alive.append(t)
        return _lib.ptr(t)

    with torch.cuda.device(dev):
        time_ptr = None if times is None else [dev_array(a, torch.int32) for a in times]
        flag_ptr = {}                                            # one upload per flag array, however many triples share it

        def flags(f):
            if f is None:
                return None
            if id(f) not in flag_ptr:
                flag_ptr[id(f)] = dev_array(_flags_u8(f, dev), torch.uint8)
            return flag_ptr[id(f)]

        ptr = _lib.ptr
        tab = (_lib.HgtViewTriple * (M + 1))()
        for m, ((tt, st, rel), (ip, src, tm)) in enumerate(zip(dgraph.tri_types, dgraph.csr_dev)):
            tf, sf = (None, None) if table is None else table[m]
            tab[m] = _lib.HgtViewTriple(ip.data_ptr(), ptr(src), ptr(tm), flags(tf), flags(sf),
                                        None if time_ptr is None else time_ptr[tt], None if time_ptr is None else time_ptr[st],
                                        int(first[m]), dgraph.n_nodes[tt], int(type_off[tt]), int(type_off[st]), rel)
        tab[M] = _lib.HgtViewTriple(None, None, None, None, None, None, None, int(first[M]), N, 0, 0, R - 1)
        tab_dev = _lib.table_to_device(tab, dev)
        has_time = times is not None
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
        i64 = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
        src32, dst32, time32 = i32(E_cap), i32(E_cap), (i32(E_cap) if has_time else None)
        ei, et, tm64 = i64(2, E_cap), i64(E_cap), (i64(E_cap) if has_time else None)
        head = i32(R + 2)
        # (the one read-back of a FILTERED view, rel_ptr and the flag word; an unfiltered view touches no pinned memory)
        head_host = _lib.pinned("view_head", _lib.HGT_SAMPLER_MAX_TRIPLES + 3, torch.int32) if filtered else None
        lib = _lib.load()
        need = C.c_uint64()
        _lib.check(lib.hgt_view_tmp_bytes(E_cap, C.byref(need)), "hgt_view_tmp_bytes")
        tmp = torch.empty(int(need.value) if filtered else 0, dtype=torch.uint8, device=dev)
        mt = 0 if max_time is None else max(-2 ** 31, min(2 ** 31 - 1, int(max_time)))
        stream = torch.cuda.current_stream(dev)
        _lib.check(lib.hgt_view_build(tab_dev.data_ptr(), M, R, E_cap, int(filtered), int(max_time is not None), mt, int(has_time),
                                      ptr(src32), ptr(dst32), ptr(time32), ptr(ei), E_cap, ptr(et), ptr(tm64), head.data_ptr(),
                                      ptr(tmp), tmp.numel(), ptr(head_host), stream.cuda_stream), "hgt_view_build")
        # (the table, the scratch and the uploaded copies were allocated on this stream: the allocator hands their memory to later
        #  work of the same stream only, so they may go out of scope here)
        E = E_cap
        if filtered:
            stream.synchronize()                                 # the one host read of a filtered view: rel_ptr and the flag word
            E, flag = int(head_host[R]), int(head_host[R + 1])
            if flag & _lib.HGT_VIEW_BAD_TIME:
                raise IndexError("pyhgt_amd: whole_graph: a time difference outside [0, %d)" % _lib.HGT_RTE_LEN)
            src32, dst32, et = src32[:E], dst32[:E], et[:E]
            time32, tm64 = (time32[:E], tm64[:E]) if has_time else (None, None)
        ei = ei[:, :E]
        node_type = torch.repeat_interleave(torch.arange(T, device=dev), torch.as_tensor(dgraph.n_nodes, dtype=torch.int64, device=dev),
                                            output_size=N)
        out = _WholeDeviceGraph((node_feature, node_type, tm64, ei, et, _node_dict(dgraph), dict(dgraph.edge_dict)))
        rel_ptr = head[:R + 1]
        type_off_d = torch.from_numpy(type_off.astype(np.int32)).to(dev)
        out.sorted = (src32, dst32, time32, rel_ptr, type_off_d)
        out._n_nodes = dict(zip(dgraph.types, dgraph.n_nodes))
        out.filtered, out._head, out._bad = filtered, head, (0 if filtered else None)
        if plan:
            out.plan = GraphPlan.from_sorted(node_type, ei, et, tm64, src32, dst32, time32, rel_ptr, type_off_d, T, R)
            GraphPlan.register(out.plan, node_type, ei, et, tm64, T, R)
    return out
