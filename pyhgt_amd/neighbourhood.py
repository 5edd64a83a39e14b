"""Exact L-hop neighbourhood of a seed set from a resident graph (csrc/hgt_neighbourhood.hip): the exact L-layer output of a few nodes
at a cost that follows the size of their neighbourhood, not the size of the graph.

`DeviceHeteroGraph.whole_graph()` followed by `gnn(*view[:5], seeds=...)` is exact, but the view, the trim's hop rounds and its outputs
are all proportional to the whole graph.  The in-edge CSRs of a `DeviceHeteroGraph` (row = target, entries = sources) are the
structure for the other way round: a frontier walk from the seeds along in-edges visits precisely the rows the seed trim keeps.

The rule is the composition of the two existing definitions, array for array:

    a    = np_whole_graph(dgraph, node_time, max_time, leave_out, self_loops)
    t    = np_trim_to_seeds(N, a.edge_index, seed_rows, n_layers)          # seed_rows = type_off[type] + id
    g    = np_trim_graph(t, a.node_type, a.edge_index, a.edge_type, a.edge_time)
    feat = a.node_feature[t.order]

  rows      in (hop, type in `dgraph.types` order, id) order: level 0 = the distinct seeds, level h + 1 = the sources of the kept
            entries of level h's rows that no earlier level holds.
  edges     in (hop of the target, position in the view) order: triples in `dgraph.triples` order, inside a triple the target rows
            ascending, a row's entries in stored order with the filtered entries gone, and last the self loops of that hop bucket in
            row order.  Level L is numbered but not expanded.
  filter    the view's: max_time / TIME_NONE / leave_out decide which entries are kept (and so which nodes are reached); edge_type,
            edge_time and the time-difference range check are the view's.
  counts    n_rows[k] = the rows of levels 0 .. L - k; n_edges[l] = the edges whose target's level is <= L - l (n_edges[0] =
            n_edges[1]): the trim's.

`np_neighbourhood` is that rule as its own frontier walk on `dgraph.csr`: it never forms the whole graph.  It returns no `hop` /
`new_id` over N and no `edge_order`: those are whole-graph-sized, and the position of an edge in a filtered view cannot be known
without counting the whole view.

The device build keeps ONE resident int32 mark per node with the graph (-1 idle; a node's new row during a call), allocated and cleared
on first use and put back at the end of every call -- and on its error paths -- by a kernel that walks the call's own row lists; a
"dirty" flag on the graph forces a full clear if a call was interrupted in between.  Calls on one graph are therefore NOT reentrant.
After the first call no launch has a grid or a loop proportional to the graph's N or E and nothing of that size is allocated --
given that the per-node tables of the call (node_time, leave_out flags) are ones the graph has seen: they are validated, converted
to int32 / uint8 and uploaded once per OBJECT and kept with the graph under its identity (`_resident`); a new object costs work of
its type's size, and a table changed in place needs `dgraph.forget_neighbourhood_tables()`.
Host reads: ONE per level that has rows, through pinned memory -- at most n_layers + 1 per call -- plus one for every int64 DEVICE
node_time table on the call that first sees it (its int32 range check); `host_reads` counts them all.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .sampler import _host_array
from .trim import TrimmedGraph, _check_layers
from .view import (_RTE_SELF, _feature_width, _flags_u8, _is_device, _leave_out_table, _node_time_tables, _np_kept, _np_time_diff,
                   _type_off)

__all__ = ["np_neighbourhood", "neighbourhood", "NeighbourhoodGraph", "NeighbourhoodArrays", "NB_CHUNK", "NB_WAVE_ROWS"]

NB_CHUNK = _lib.HGT_NB_CHUNK            # entries of a row one wavefront takes; a longer row is split into chunks
NB_WAVE_ROWS = _lib.HGT_NB_WAVE_ROWS    # rows of a level whose totals one wavefront of the numbering kernel sums
_LIMIT = 2 ** 31 - 1

NeighbourhoodArrays = namedtuple("NeighbourhoodArrays",
                                 "order node_type edge_index edge_type edge_time node_feature out_rows n_rows n_edges row_id")


# ------------------------------------------------------------------------------------------------------------ arguments
def _seed_lists(dgraph, seeds):
    """seeds = {type name: ids} -> [(type index, ids)] in the dict's order; ids an int64 numpy array (checked against the type's
    nodes: IndexError) or, for a device tensor, an int64 device tensor (checked by the build).  KeyError: an unknown type."""
    if seeds is None:
        seeds = {}
    unknown = [t for t in seeds if t not in dgraph.types]
    if unknown:
        raise KeyError("pyhgt_amd: seed types %r are not node types of the graph" % (unknown,))
    out = []
    for name, ids in seeds.items():
        t = dgraph.types.index(name)
        if _is_device(ids):
            if ids.dtype not in (torch.int32, torch.int64):
                raise TypeError("pyhgt_amd: seed ids of %r must be integers" % name)
            out.append((t, ids.to(torch.int64).reshape(-1)))
            continue
        a = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
        if a.size == 0:
            a = a.astype(np.int64)
        if a.dtype.kind not in "iu":
            raise TypeError("pyhgt_amd: seed ids of %r must be integers" % name)
        a = a.astype(np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= dgraph.n_nodes[t]):
            raise IndexError("pyhgt_amd: seed ids of %r outside [0, %d)" % (name, dgraph.n_nodes[t]))
        out.append((t, a))
    return out


def _check_caps(level, rows, edges, max_rows, max_edges):
    if max_rows is not None and rows > max_rows:
        raise OverflowError("pyhgt_amd: neighbourhood: %d rows at hop level %d, max_rows is %d" % (rows, level, max_rows))
    if max_edges is not None and edges > max_edges:
        raise OverflowError("pyhgt_amd: neighbourhood: %d edges at hop level %d, max_edges is %d" % (edges, level, max_edges))


def _counts(L, n_level, e_level):
    """per-level rows [L + 1] and edges [L] -> the trim's (n_rows, n_edges)"""
    rows, edges = np.cumsum(n_level), np.cumsum(e_level)
    n_rows = tuple(int(rows[L - k]) for k in range(L + 1))
    ne = [int(edges[L - l]) for l in range(1, L + 1)]
    return n_rows, tuple([ne[0]] + ne)


# ------------------------------------------------------------------------------------------------------------ the definition
def np_neighbourhood(dgraph, seeds, n_layers, node_time=None, max_time=None, leave_out=None, self_loops=True):
    """The definition (module docstring) as a frontier walk on `dgraph.csr`.  seeds = {type name: ids}, any order, repeats allowed;
    the dict's order is the order of `out_rows`.  -> NeighbourhoodArrays: order int64[n_rows[0]] (the view row of every new row),
    node_type, edge_index int64[2, n_edges[1]], edge_type, edge_time (None without node_time), node_feature float32[n_rows[0], width]
    (None for a graph without features), out_rows int64[len(seeds)], n_rows, n_edges (tuples, indexed by the layer) and row_id (the id
    inside its type of every row).

    KeyError: an unknown seed type or `leave_out` triple.  IndexError: a seed id outside its type; a kept edge of the neighbourhood
    whose time difference is outside [0, 240).  ValueError: n_layers outside [1, HGT_TRIM_MAX_LAYERS], the view's node_time rules,
    feature widths that differ."""
    L = _check_layers(n_layers)
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    times = _node_time_tables(dgraph, node_time)
    if times is not None:
        times = [a.cpu().numpy().astype(np.int64) if isinstance(a, torch.Tensor) else a for a in times]
    table = _leave_out_table(dgraph, leave_out)
    seed_lists = [(t, a.cpu().numpy() if isinstance(a, torch.Tensor) else a) for t, a in _seed_lists(dgraph, seeds)]
    for t, a in seed_lists:
        if a.size and (a.min() < 0 or a.max() >= dgraph.n_nodes[t]):
            raise IndexError("pyhgt_amd: seed ids of %r outside [0, %d)" % (dgraph.types[t], dgraph.n_nodes[t]))
    feats = dgraph.features_host
    width = None if feats is None else _feature_width(dgraph.n_nodes, feats, dgraph.types)
    type_off = _type_off(dgraph)
    mark = [np.full(n, -1, np.int64) for n in dgraph.n_nodes]
    by_target = [[m for m, (tt, _, _) in enumerate(dgraph.tri_types) if tt == t] for t in range(T)]
    csr = dgraph.csr

    level = [np.unique(np.concatenate([a for t, a in seed_lists if t == tt] + [np.zeros(0, np.int64)])) for tt in range(T)]
    row_type, row_id, n_level, e_level = [], [], [], []
    e_src, e_dst, e_type, e_time = [], [], [], []
    base = 0
    for h in range(L + 1):
        first = base                                            # numbers: level offset + rank in (type, id) order
        for t in range(T):
            ids = level[t]
            mark[t][ids] = base + np.arange(ids.size)
            row_type.append(np.full(ids.size, t, np.int64)); row_id.append(ids)
            base += ids.size
        n_level.append(base - first)
        if h == L:
            break
        found = [[] for _ in range(T)]
        pending = []                                            # (source type, source ids, new target rows, relation, times)
        for m, (tt, st, rel) in enumerate(dgraph.tri_types):    # triple-major: the view's order
            ids = level[tt]
            if ids.size == 0:
                continue
            indptr, src, time = csr[m]
            deg = (indptr[ids + 1] - indptr[ids]).astype(np.int64)
            rows = np.repeat(ids, deg)
            pos = np.repeat(indptr[ids].astype(np.int64) - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg) + np.arange(int(deg.sum()))
            s = src[pos].astype(np.int64)
            keep = _np_kept(time[pos], rows, s, None if times is None else times[tt], max_time, None if table is None else table[m])
            rows, s = rows[keep], s[keep]
            dt = None
            if times is not None:
                dt = _np_time_diff(times[tt], times[st], rows, s, "neighbourhood: a time difference of %r" % (dgraph.triples[m],))
            pending.append((st, s, mark[tt][rows], rel, dt))
            found[st].append(s[mark[st][s] < 0])
        level = [np.unique(np.concatenate(f + [np.zeros(0, np.int64)])) for f in found]
        for t in range(T):                                      # the next level's numbers, which this level's edges name
            mark[t][level[t]] = base + sum(level[u].size for u in range(t)) + np.arange(level[t].size)
        count = 0
        for st, s, dst, rel, dt in pending:
            e_src.append(mark[st][s]); e_dst.append(dst); e_type.append(np.full(s.size, rel, np.int64))
            if times is not None:
                e_time.append(dt)
            count += s.size
        if self_loops:
            loops = np.arange(first, base, dtype=np.int64)
            e_src.append(loops); e_dst.append(loops); e_type.append(np.full(loops.size, R - 1, np.int64))
            if times is not None:
                e_time.append(np.full(loops.size, _RTE_SELF, np.int64))
            count += loops.size
        e_level.append(count)
    cat = lambda a: np.concatenate(a).astype(np.int64) if a else np.zeros(0, np.int64)
    row_type, row_id = cat(row_type), cat(row_id)
    n_rows, n_edges = _counts(L, n_level, e_level)
    order = type_off[row_type] + row_id
    feature = None
    if feats is not None:
        feature = np.zeros((row_type.size, width), np.float32)
        for t in range(T):
            sel = row_type == t
            if sel.any():
                feature[sel] = _host_array(feats[t])[row_id[sel]]
    out_rows = cat([mark[t][a] for t, a in seed_lists])
    return NeighbourhoodArrays(order, row_type, np.stack([cat(e_src), cat(e_dst)]), cat(e_type), cat(e_time) if times is not None else None,
                               feature, out_rows, n_rows, n_edges, row_id)


# ------------------------------------------------------------------------------------------------------------ the result
class NeighbourhoodGraph(TrimmedGraph):
    """Result of `DeviceHeteroGraph.neighbourhood`: a `TrimmedGraph` whose rows are already gathered.  Everything `gnn(..., trim=nb)`
    uses -- n_layers, n_rows, n_edges, n_seeds, num_types, num_relations, node_type, edge_index, edge_type, edge_time, out_rows,
    layer_graph(l), plan(l, use_rte) -- and `node_feature` float32[n_rows[0], width] (the rows' features, in the rows' order),
    `order` (the whole-graph view's row of every row), `row_id` (the id inside its type), `seed_rows(type)`, `inputs` = (node_feature,
    node_type, edge_time, edge_index, edge_type): `gnn(*nb.inputs, trim=nb)`.  It has no hop / new_id / edge_order: those are
    whole-graph-sized.  `host_reads` = the host reads its build made."""
    gathered = True
    host_reads = 0

    @property
    def inputs(self):
        return (self.node_feature, self.node_type, self.edge_time, self.edge_index, self.edge_type)

    def seed_rows(self, type_name):
        """the slice of the result (and of `out_rows`) that belongs to the seeds of a type"""
        return self._seed_slices[type_name]


def _finish(nb, dgraph, L, seed_lists, n_rows, n_edges):
    nb.n_layers, nb.n_rows, nb.n_edges = L, tuple(n_rows), tuple(n_edges)
    nb.n_nodes = nb.n_rows[0]                                 # the graph `gnn(*nb.inputs, trim=nb)` is called with
    nb.num_types, nb.num_relations = len(dgraph.types), len(dgraph.edge_dict)
    nb._seed_slices, at = {}, 0
    for t, a in seed_lists:
        n = int(a.numel() if isinstance(a, torch.Tensor) else a.size)
        nb._seed_slices[dgraph.types[t]] = slice(at, at + n)
        at += n
    nb.n_seeds = at
    return nb


def _host_neighbourhood(dgraph, seeds, L, node_time, max_time, leave_out, self_loops, max_rows, max_edges):
    a = np_neighbourhood(dgraph, seeds, L, node_time, max_time, leave_out, self_loops)
    if a.node_feature is None and a.node_type.size:
        raise ValueError("pyhgt_amd: the DeviceHeteroGraph carries no features")
    for h in range(L + 1):                                    # level by level, as the device build meets its caps
        _check_caps(h, a.n_rows[L - h], a.n_edges[L - h + 1] if h >= 1 else 0, max_rows, max_edges)
    tt = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x))
    nb = NeighbourhoodGraph()
    nb.node_feature = tt(np.zeros((0, 0), np.float32) if a.node_feature is None else a.node_feature)
    nb.order, nb.row_id, nb.node_type, nb.out_rows = tt(a.order), tt(a.row_id), tt(a.node_type), tt(a.out_rows)
    nb.edge_index, nb.edge_type, nb.edge_time = tt(a.edge_index), tt(a.edge_type), tt(a.edge_time)
    return _finish(nb, dgraph, L, _seed_lists(dgraph, seeds), a.n_rows, a.n_edges)


# ------------------------------------------------------------------------------------------------------------ the device build
def _marks(dgraph):
    """the resident marks: allocated and cleared on first use; cleared again in full if a call was interrupted"""
    dev = dgraph.device
    if dgraph._nb_mark is None:
        dgraph._nb_mark = [torch.full((n,), -1, dtype=torch.int32, device=dev) for n in dgraph.n_nodes]
        dgraph._nb_dirty = False
    elif dgraph._nb_dirty:
        for m in dgraph._nb_mark:
            m.fill_(-1)
        dgraph._nb_dirty = False
    return dgraph._nb_mark


_TABLES_KEPT = 64


def _resident(dgraph, obj, kind, make):
    """The device form of a caller's per-node table (`kind`: "time" -> int32, "flags" -> uint8), kept with the graph under the
    IDENTITY of the caller's object (which is held, so its id stays its own): the first call with an object validates, converts and
    uploads it -- work of the type's size -- and every later call with the same object touches nothing of that size.  -> (tensor,
    made now)"""
    cache = dgraph._nb_tables
    hit = cache.get((id(obj), kind))
    if hit is not None and hit[0] is obj:
        return hit[1], False
    if len(cache) >= _TABLES_KEPT:
        cache.clear()
    t = make()
    cache[(id(obj), kind)] = (obj, t)
    return t, True


def _resident_times(dgraph, node_time, dev):
    """node_time -> (per type an int32 device tensor, or None for no tables; the host reads this made).  Tables this graph has seen
    (by object) are taken as they were validated then; otherwise the view's checks run on all of them (`_node_time_tables`: an int64
    device tensor costs one host read for its range) and the int32 device forms are kept."""
    if not node_time:
        return None, 0
    cache = dgraph._nb_tables
    objs = [node_time.get(t) for t in dgraph.types]
    seen = lambda o: cache.get((id(o), "time"), (None,))[0] is o
    if set(node_time) <= set(dgraph.types) and all(n == 0 or (o is not None and seen(o)) for o, n in zip(objs, dgraph.n_nodes)):
        return [cache[(id(o), "time")][1] if n else torch.zeros(0, dtype=torch.int32, device=dev) for o, n in zip(objs, dgraph.n_nodes)], 0
    tables = _node_time_tables(dgraph, node_time)
    reads = sum(1 for a in tables if _is_device(a) and a.dtype == torch.int64 and a.numel())
    out = []
    for o, a in zip(objs, tables):
        up = lambda a=a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=torch.int32).contiguous()
        out.append(up() if o is None else _resident(dgraph, o, "time", up)[0])
    return out, reads


def neighbourhood(dgraph, seeds, n_layers, node_time=None, max_time=None, leave_out=None, self_loops=True, max_rows=None, max_edges=None):
    """`DeviceHeteroGraph.neighbourhood` (its docstring has the interface; the module docstring the rule)."""
    L = _check_layers(n_layers)
    if dgraph.device is None:
        return _host_neighbourhood(dgraph, seeds, L, node_time, max_time, leave_out, self_loops, max_rows, max_edges)
    if dgraph.device.type != "cuda":
        raise RuntimeError("pyhgt_amd: neighbourhood builds on a GPU (no CPU fallback; a host-only graph gets the numpy definition)")
    dev = dgraph.device
    T, R, M = len(dgraph.types), len(dgraph.edge_dict), len(dgraph.triples)
    times, reads = _resident_times(dgraph, node_time, dev)
    table = _leave_out_table(dgraph, leave_out)
    seed_lists = _seed_lists(dgraph, seeds)
    if dgraph.features is None:
        raise ValueError("pyhgt_amd: the DeviceHeteroGraph carries no features")
    width = _feature_width(dgraph.n_nodes, dgraph.features, dgraph.types)
    type_off = _type_off(dgraph)
    has_time = times is not None
    lib = _lib.load()
    i64 = lambda *shape: torch.empty(*shape, dtype=torch.int64, device=dev)
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    ptr = _lib.ptr
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        st = stream.cuda_stream
        marks = _marks(dgraph)
        time_ptr = None if times is None else [ptr(a) for a in times]

        def flags(f):
            """a leave-out array as resident uint8 on the device: one conversion and upload per OBJECT, then nothing of its size"""
            if f is None:
                return None
            return ptr(_resident(dgraph, f, "flags", lambda: _flags_u8(f, dev))[0])

        types_c = (_lib.HgtNbType * T)()
        for t in range(T):
            f = dgraph.features[t]
            types_c[t] = _lib.HgtNbType(ptr(marks[t]), None if f is None or dgraph.n_nodes[t] == 0 else f.data_ptr(),
                                        0 if f is None else f.stride(0), int(type_off[t]), dgraph.n_nodes[t], 0)
        tri_c = (_lib.HgtNbTriple * max(M, 1))()
        for m, ((tt, s_t, rel), (ip, src, tm)) in enumerate(zip(dgraph.tri_types, dgraph.csr_dev)):
            tf, sf = (None, None) if table is None else table[m]
            tri_c[m] = _lib.HgtNbTriple(ip.data_ptr(), ptr(src), ptr(tm), flags(tf), flags(sf),
                                        None if time_ptr is None else time_ptr[tt], None if time_ptr is None else time_ptr[s_t],
                                        tt, s_t, rel, 0)
        types_dev, tri_dev = _lib.table_to_device(types_c, dev), _lib.table_to_device(tri_c, dev)
        S = sum(int(a.numel() if isinstance(a, torch.Tensor) else a.size) for _, a in seed_lists)
        if S >= _LIMIT:
            raise ValueError("pyhgt_amd: neighbourhood takes fewer than 2^31 - 1 seeds")
        if S:
            seed_id = torch.cat([(a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).to(dev) for _, a in seed_lists])
            seed_type = torch.cat([torch.full((int(a.numel() if isinstance(a, torch.Tensor) else a.size),), t, dtype=torch.int32)
                                   for t, a in seed_lists]).to(dev)
        else:
            seed_id, seed_type = i64(0), i32(0)
        head = i64(_lib.HGT_NB_HEAD_WORDS)
        host = _lib.pinned("nb_head", _lib.HGT_NB_HEAD_WORDS, torch.int64)   # (each read waits for its copy before the next is issued)
        mt = 0 if max_time is None else max(-2 ** 31, min(2 ** 31 - 1, int(max_time)))
        keys, rows_out, edges_out = [], [], []              # per level: sorted key list; (order, node_type, row_id); (src, dst, type, time)
        n_level, e_level = [], []

        def read():
            host.copy_(head, non_blocking=True)
            done = torch.cuda.Event()
            done.record(stream)
            done.synchronize()
            return host.tolist()

        def number(cand, cap, row_base, expand):
            need = C.c_uint64()
            _lib.check(lib.hgt_nb_sort_bytes(cap, T, C.byref(need)), "hgt_nb_sort_bytes")
            tmp = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
            k, out = i64(cap), (i64(cap), i64(cap), i64(cap))
            keys.append(k)                                     # (in the list before the launch: an error path resets by it)
            _lib.check(lib.hgt_nb_number(types_dev.data_ptr(), T, tri_dev.data_ptr(), M, cand.data_ptr(), cap, k.data_ptr(), tmp.data_ptr(),
                                         tmp.numel(), row_base, int(expand), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                         head.data_ptr(), st), "hgt_nb_number")
            rows_out.append(out)

        def reset():
            for k in keys:
                _lib.check(lib.hgt_nb_reset(types_dev.data_ptr(), T, k.data_ptr(), k.numel(), st), "hgt_nb_reset")
            dgraph._nb_dirty = False

        dgraph._nb_dirty = True                                # until the marks have been walked back
        if S:
            cand = i64(S)
            _lib.check(lib.hgt_nb_seeds(types_dev.data_ptr(), T, seed_type.data_ptr(), seed_id.data_ptr(), S, cand.data_ptr(),
                                        head.data_ptr(), st), "hgt_nb_seeds")
            number(cand, S, 0, True)
            h0 = read(); reads += 1
        else:
            h0 = [0] * _lib.HGT_NB_HEAD_WORDS
        try:
            if h0[_lib.HGT_NB_HEAD_FLAGS] & _lib.HGT_NB_BAD_SEED:
                raise IndexError("pyhgt_amd: neighbourhood: a seed id outside its type's nodes")
            hd = h0
            n_level.append(int(hd[_lib.HGT_NB_HEAD_N]))
            _check_caps(0, n_level[0], 0, max_rows, max_edges)
            for h in range(L):
                n_h, base = n_level[h], sum(n_level[:h])
                if n_h == 0:
                    n_level.append(0); e_level.append(0); edges_out.append(None)
                    continue
                deg, chunks = int(hd[_lib.HGT_NB_HEAD_DEG]), int(hd[_lib.HGT_NB_HEAD_CHUNKS])
                e_cap = deg + (n_h if self_loops else 0)
                if e_cap >= _LIMIT or base + n_h + deg >= _LIMIT:
                    raise OverflowError("pyhgt_amd: neighbourhood: hop level %d has %d CSR entries; a level takes fewer than 2^31 - 1" % (h, deg))
                if max_edges is not None and max_time is None and table is None:
                    _check_caps(h, base + n_h, sum(e_level) + e_cap, max_rows, max_edges)   # (unfiltered: every entry is kept)
                tb = (C.c_int64 * T)(*hd[_lib.HGT_NB_HEAD_TYPE_BEGIN:_lib.HGT_NB_HEAD_TYPE_BEGIN + T])
                te = (C.c_int64 * T)(*hd[_lib.HGT_NB_HEAD_TYPE_END:_lib.HGT_NB_HEAD_TYPE_END + T])
                n_items = sum(te[tt] - tb[tt] for tt, _, _ in dgraph.tri_types)
                item_chunks, item_entries, chunk_cnt = i32(n_items + 1), i32(n_items + 1), i32(chunks + 1)
                cand = i64(max(deg, 1))
                lvl = keys[h]
                _lib.check(lib.hgt_nb_expand(types_dev.data_ptr(), T, tri_dev.data_ptr(), C.addressof(tri_c), M, lvl.data_ptr(), tb, te, n_h,
                                             chunks, int(max_time is not None), mt, item_chunks.data_ptr(), item_entries.data_ptr(),
                                             chunk_cnt.data_ptr(), cand.data_ptr(), deg, head.data_ptr(), st), "hgt_nb_expand")
                if deg > 0:
                    number(cand, deg, base + n_h, h + 1 < L)
                eo = (i64(e_cap), i64(e_cap), i64(e_cap), i64(e_cap) if has_time else None)
                _lib.check(lib.hgt_nb_fill(types_dev.data_ptr(), T, tri_dev.data_ptr(), C.addressof(tri_c), M, lvl.data_ptr(), tb, te, n_h,
                                           chunks, int(max_time is not None), mt, int(has_time), int(bool(self_loops)), R - 1, base,
                                           item_chunks.data_ptr(), chunk_cnt.data_ptr(), ptr(eo[0]), ptr(eo[1]), ptr(eo[2]), ptr(eo[3]),
                                           e_cap, head.data_ptr(), st), "hgt_nb_fill")
                edges_out.append(eo)
                if deg > 0:
                    hd = read(); reads += 1
                    if hd[_lib.HGT_NB_HEAD_FLAGS] & _lib.HGT_NB_BAD_TIME:
                        raise IndexError("pyhgt_amd: neighbourhood: a time difference outside [0, %d)" % _lib.HGT_RTE_LEN)
                    n_level.append(int(hd[_lib.HGT_NB_HEAD_N]))
                    e_level.append(int(hd[_lib.HGT_NB_HEAD_KEPT]) + (n_h if self_loops else 0))
                else:
                    n_level.append(0)
                    e_level.append(n_h if self_loops else 0)
                _check_caps(h + 1, sum(n_level), sum(e_level), max_rows, max_edges)
            # ---- the result: the levels' pieces joined (sizes of the neighbourhood), the features, the seeds' rows
            n_rows, n_edges = _counts(L, n_level, e_level)
            n0 = n_rows[0]
            join = lambda parts: torch.cat(parts) if parts else i64(0)
            order, node_type, row_id = (join([rows_out[h][i][:n_level[h]] for h in range(len(rows_out)) if n_level[h]]) for i in range(3))
            epieces = [(edges_out[h], e_level[h]) for h in range(L) if edges_out[h] is not None and e_level[h]]
            src, dst, etype = (join([eo[i][:n] for eo, n in epieces]) for i in range(3))
            etime = join([eo[3][:n] for eo, n in epieces]) if has_time else None
            feature = torch.empty(n0, width, dtype=torch.float32, device=dev)
            out_rows = i64(S)
            _lib.check(lib.hgt_nb_finish(types_dev.data_ptr(), T, ptr(node_type), ptr(row_id), n0, width, ptr(feature), ptr(seed_type),
                                         ptr(seed_id), S, ptr(out_rows), st), "hgt_nb_finish")
        except (IndexError, OverflowError):                    # raised at a read: every claimed node stands in a sorted list
            reset()
            raise                                              # (anything else leaves the graph dirty: the next call clears in full)
        reset()
    nb = NeighbourhoodGraph()
    nb.node_feature, nb.order, nb.row_id, nb.node_type, nb.out_rows = feature, order, row_id, node_type, out_rows
    nb.edge_index, nb.edge_type, nb.edge_time = torch.stack([src, dst]), etype, etime
    nb.host_reads = reads
    return _finish(nb, dgraph, L, seed_lists, n_rows, n_edges)
