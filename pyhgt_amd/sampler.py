"""HGSampling on the device (csrc/hgt_sampler.hip): the producer of the sampled batches.

The reference draws a training batch with `sample_subgraph` + `to_torch` (pyHGT/data.py:87-256): Python dict walking on the CPU,
seconds per batch.  Here the graph lives in device memory (`DeviceHeteroGraph`: one CSR by target id per meta triple, one feature
matrix per type) and `sample_subgraph_device` turns seed nodes into the `_DeviceGraph` that `to_device_graph` would have built --
the 7-tuple of `to_torch` with `.sorted`, `.plan` and `.indxs` -- with one host synchronisation per batch (the sizes of the
result) and no host copy of an index.  `sample_subgraph_host` is its numpy sibling with the same definition: the same Philox words,
the same fixed-point scores, selection keys in float64.

The definition ("Device sampler", lists where it departs from the reference):

  step     seeds of type j (get_types() order): step j;  layer l, type j: step T * (1 + l) + j.  Types are visited in get_types() order.
  budget   data.py:112-130 per newly sampled node and meta triple into its type: all neighbours if degree <= sampled_number, else the
           sampled_number neighbours with the smallest (Philox word, position); a neighbour whose time is None inherits the target's;
           neighbours newer than max_time or already sampled are skipped; the others get score += round(2^32 / len(subset)) (u64,
           32.32 fixed point) and stamp = max(stamp, (step << 32) | (time ^ 0x80000000)).
  select   data.py:151-172: the min(sampled_number, candidates) candidates with the smallest (key, node id),
           key = -log(u) / s^2, s = score * 2^-32, u = ((word >> 8) + 0.5) * 2^-24 (exponential keys of Efraimidis and Spirakis: the
           ordered sample is distributed like successive weighted sampling without replacement, i.e. like
           np.random.choice(p = score^2 / sum, replace = False)).  Serials follow that order; the node's time is its stamp's.
  induce   data.py:183-209, 240-250: relation-major edges, inside a relation by global target id, a target's neighbours in adjacency
           order, `self` edges last; edge_time = time[tgt] - time[src] + 120.
  mask     (task batches, OAG/train_paper_field.py:109-122) mask = {(target type, source type, relation): (tgt_below, src_below)}: an
           edge of that triple between the sampled target of serial i and a sampled source of serial ser is left out iff
           i < tgt_below or ser < src_below.  Serials are per type and the seeds of a type are its first serials in the order given;
           `self` edges are never masked; nothing else changes.  `np_induce` is the definition, `seed_edge_mask` builds the dict.

Labels of a task batch come from the same relation of the full graph: `LabelSpace` (csrc/hgt_sampler_labels.hip on a device graph, the
`np_label_*` siblings on the host).

Batched calls: `sample_subgraphs_device` draws B sub-graphs that share nothing but the resident graph in one pass of the launches of a
single call (replica b = blockIdx.y of every launch) with one host read; element b is bit for bit what `sample_subgraph_device` returns
for (inps[b], seeds[b]).  `sample_subgraphs_host` is the definition: the list of the single host calls.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .conv import GraphPlan
from .sampled import _DeviceGraph

__all__ = ["DeviceHeteroGraph", "sample_subgraph_device", "sample_subgraph_host", "sample_subgraphs_device", "sample_subgraphs_host",
           "philox4x32_10", "seed_edge_mask", "LabelSpace", "np_label_distribution", "np_label_index", "np_label_counts", "np_label_columns"]

TIME_NONE = _lib.HGT_SAMPLER_TIME_NONE
_SUBSET_TAG, _SELECT_TAG = 0x10000, 0x20000
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 over numpy arrays (csrc/hgt_philox.h bit for bit): counter words c0..c3 (broadcast against each other), key =
    (seed & 0xffffffff, seed >> 32) -> the four uint32 output words."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    c0, c1, c2, c3 = c
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        n0, n2 = (p1 >> s32) ^ c1 ^ k0, (p0 >> s32) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & _MASK, p0 & _MASK, n0, n2
        k0, k1 = (k0 + w0) & _MASK, (k1 + w1) & _MASK
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def _bias(t):
    return (np.asarray(t, dtype=np.int64) + 2 ** 31).astype(np.uint64)


def _stamp_time(stamp):
    return ((np.asarray(stamp, dtype=np.uint64) & _MASK).astype(np.int64) - 2 ** 31).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- the graph
class DeviceHeteroGraph:
    """A heterogeneous graph resident on a device (or, device=None, on the host only -- what `sample_subgraph_host` needs).

    types       node type names in get_types() order
    triples     [(target type, source type, relation)] without `self`, ordered by (relation id, target type); the position in this
                list is the triple's index in the random-word keys
    csr         per triple (indptr int32[n_tgt + 1], src int32[], time int32[]), TIME_NONE = the reference's None
    features    per type a float32 [n_type, in_dim] matrix (or None for a type without nodes)
    degree      {type: int32 [n_type]}: neighbours summed over the triples into the type
    Three ways in: from_csr (finished CSRs), from_reference_graph (the reference's nested dicts) and from_edge_lists (raw edge lists;
    with a device the CSRs are built there and `csr` is downloaded on first use -- pyhgt_amd/graph_build.py).
    It answers get_types() / get_meta_graph() like the reference's Graph, so it can stand in for `graph` in to_torch-like calls."""

    def __init__(self, types, meta, n_nodes, csr, features=None, device=None):
        meta = [tuple(m) for m in meta]
        if len(meta) != len(csr):
            raise ValueError("pyhgt_amd: one CSR per meta triple")
        picked = self._set_schema(types, meta, n_nodes)
        tid = {t: i for i, t in enumerate(self.types)}
        self._csr = []
        for i in picked:
            indptr, src, time = csr[i]
            tt, st, _ = meta[i]
            indptr = np.ascontiguousarray(indptr, dtype=np.int32)
            src = np.ascontiguousarray(src, dtype=np.int32)
            time = np.full(src.shape, TIME_NONE, np.int32) if time is None else np.ascontiguousarray(time, dtype=np.int32)
            if indptr.shape != (self.n_nodes[tid[tt]] + 1,) or indptr[0] != 0 or np.any(np.diff(indptr) < 0) or indptr[-1] != src.size:
                raise ValueError("pyhgt_amd: indptr of %r is not a CSR over the target type's nodes" % (meta[i],))
            if time.shape != src.shape or (src.size and (src.min() < 0 or src.max() >= self.n_nodes[tid[st]])):
                raise ValueError("pyhgt_amd: neighbour ids / times of %r out of range" % (meta[i],))
            self._csr.append((indptr, src, time))
        self.device = None if device is None else torch.device(device)
        if self.device is not None:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            self.csr_dev = [tuple(up(a) for a in c) for c in self._csr]
        self.set_features(features)

    def _set_schema(self, types, meta, n_nodes):
        """types / meta / edge_dict / triples / tri_types and the empty call state; -> the positions in `meta` of the triples, in the
        order of `triples` (by relation id, then target type; `self` left out, data.py:116)"""
        self.types = list(types)
        T = len(self.types)
        if not 1 <= T <= _lib.HGT_SAMPLER_MAX_TYPES:
            raise ValueError("pyhgt_amd: 1..%d node types, got %d" % (_lib.HGT_SAMPLER_MAX_TYPES, T))
        keep = [i for i, m in enumerate(meta) if m[2] != "self"]                    # data.py:116
        self.meta = [meta[i] for i in keep]
        if len(self.meta) > _lib.HGT_SAMPLER_MAX_TRIPLES:
            raise ValueError("pyhgt_amd: at most %d meta triples" % _lib.HGT_SAMPLER_MAX_TRIPLES)
        self.edge_dict = {m[2]: i for i, m in enumerate(self.meta)}                 # data.py:237-238
        self.edge_dict["self"] = len(self.edge_dict)
        self.n_nodes = [int(n_nodes[t]) for t in self.types]
        tid = {t: i for i, t in enumerate(self.types)}
        order = sorted(range(len(keep)), key=lambda i: (self.edge_dict[self.meta[i][2]], tid[self.meta[i][0]]))
        self.triples = [self.meta[i] for i in order]
        self.tri_types = [(tid[tt], tid[st], self.edge_dict[rel]) for tt, st, rel in self.triples]
        self._degree = None
        self._host_state = None
        self._dev_state = {}
        self._dev_nodes = None
        self._dev_dirty = False                              # the per-node device arrays hold something a reset has not walked
        self._batch_state = {}                               # the same three for batched calls (sample_subgraphs_device): [B, n] arrays
        self._batch_nodes = None                             # of their own, sized for the largest B seen, and a flag of their own
        self._batch_dirty = False
        self._nb_mark = None                                 # neighbourhood(): one resident int32 mark per node, -1 between calls,
        self._nb_dirty = False                               # and the flag that a call did not walk them back
        self._nb_tables = {}                                 # the callers' node_time / leave_out tables in their resident device form
        return [keep[i] for i in order]

    def set_features(self, features):
        """features = {type: [n_type, in_dim]} (or None): replaces the feature matrices, e.g. once `neighbour_mean` has computed those
        of the types that came without any"""
        tid = {t: i for i, t in enumerate(self.types)}
        self.features_host = None if features is None else [None if features.get(t) is None else features[t] for t in self.types]
        if self.device is not None:
            self.features = None
            if features is not None:
                self.features = []
                for t, f in zip(self.types, self.features_host):
                    f = None if f is None else torch.as_tensor(f, dtype=torch.float32).to(self.device).contiguous()
                    if f is not None and (f.dim() != 2 or f.size(0) != self.n_nodes[tid[t]]):
                        raise ValueError("pyhgt_amd: features[%r] must be [n_nodes, in_dim]" % t)
                    self.features.append(f)

    @classmethod
    def _from_device_csr(cls, types, meta, n_nodes, csr_dev, features, device):
        """The private way in for a graph whose CSRs were BUILT on the device (from_edge_lists): per meta triple contiguous int32 device
        tensors (indptr, src, time) whose invariants the building kernels guarantee -- nothing is validated or copied to the host here;
        `.csr` downloads them on first use."""
        self = cls.__new__(cls)
        picked = self._set_schema(types, [tuple(m) for m in meta], n_nodes)
        self.device = torch.device(device)
        self._csr = None
        self.csr_dev = [tuple(csr_dev[i]) for i in picked]
        self.set_features(features)
        return self

    @property
    def csr(self):
        """per triple (indptr, src, time) as host numpy arrays; of a graph built on the device: downloaded once, on first use"""
        if self._csr is None:
            self._csr = [tuple(a.cpu().numpy() for a in c) for c in self.csr_dev]
        return self._csr

    @property
    def degree(self):
        """{type: int32 [n]}: a node's neighbours summed over all triples whose target is its type (preprocess_ogbn_mag.py:63) -- device
        tensors on a device graph, numpy arrays on a host graph; log10 of it is the script's last feature column"""
        if self._degree is None:
            if self.device is not None:
                deg = [torch.zeros(n, dtype=torch.int32, device=self.device) for n in self.n_nodes]
                for (tt, _, _), (ip, _, _) in zip(self.tri_types, self.csr_dev):
                    deg[tt] += ip[1:] - ip[:-1]
            else:
                deg = [np.zeros(n, np.int32) for n in self.n_nodes]
                for (tt, _, _), (ip, _, _) in zip(self.tri_types, self.csr):
                    deg[tt] += np.diff(ip)
            self._degree = dict(zip(self.types, deg))
        return self._degree

    @classmethod
    def from_csr(cls, types, meta, n_nodes, csr, features=None, device=None):
        """types: names; meta: [(target type, source type, relation)]; n_nodes: {type: count}; csr: per triple (indptr, src, time)
        with time None or an int array in which TIME_NONE marks a missing time; features: {type: [n, in_dim]}."""
        return cls(types, meta, n_nodes, csr, features, device)

    @classmethod
    def from_reference_graph(cls, graph, features, device=None, n_nodes=None):
        """One walk over the reference's `graph.edge_list[target_type][source_type][relation][target_id][source_id] = time` into the
        CSRs, neighbours in the dict's order, a relation named `self` ignored (data.py:116).  `features`: {type: [n_type, in_dim]}, built
        once by the caller (e.g. feature_OAG over all ids); it also fixes the node counts unless n_nodes gives them."""
        types = list(graph.get_types())
        n_nodes = {t: (len(features[t]) if features.get(t) is not None else 0) for t in types} if n_nodes is None else dict(n_nodes)
        meta, csr = [], []
        for tt in graph.edge_list:
            for st in graph.edge_list[tt]:
                for rel in graph.edge_list[tt][st]:
                    if rel == "self":
                        continue
                    adj = graph.edge_list[tt][st][rel]
                    deg = np.zeros(n_nodes[tt] + 1, np.int64)
                    for v, nb in adj.items():
                        deg[int(v) + 1] = len(nb)
                    indptr = np.cumsum(deg)
                    src, time = np.empty(indptr[-1], np.int32), np.empty(indptr[-1], np.int32)
                    for v, nb in adj.items():
                        b = indptr[int(v)]
                        src[b:b + len(nb)] = list(nb.keys())
                        time[b:b + len(nb)] = [TIME_NONE if x is None else int(x) for x in nb.values()]
                    meta.append((tt, st, rel))
                    csr.append((indptr, src, time))
        return cls(types, meta, n_nodes, csr, features, device)

    @classmethod
    def from_edge_lists(cls, types, n_nodes, edges, edge_time=None, node_time=None, features=None, device=None, reverse="rev_"):
        """From raw edge lists, the form heterogeneous datasets ship in: edges = {(source type, relation, target type): edge_index [2, E]}
        (row 0 the sources), in the key order of OGB's edge_index_dict -- what ogbn-mag/preprocess_ogbn_mag.py:29-42 turns into nested
        dicts and `from_reference_graph` into CSRs, with the same result array for array.  With `device` the CSRs are built there
        (csrc/hgt_graph_build.hip) from edge arrays that never visit the host; device=None runs the numpy definition
        `np_edge_lists_to_csr`.  pyhgt_amd/graph_build.py has the arguments and the rule."""
        from .graph_build import build_from_edge_lists
        return build_from_edge_lists(cls, types, n_nodes, edges, edge_time, node_time, features, device, reverse)

    def whole_graph(self, node_time=None, max_time=None, leave_out=None, self_loops=True, plan=True):
        """The graph as the model's input, with no sampling: the 7-tuple of `to_torch` (node_feature, node_type, edge_time, edge_index,
        edge_type, node_dict, edge_dict) over ALL nodes and all edges -- or those that max_time ("the graph as of year Y") and
        leave_out (label edges) keep.  pyhgt_amd/view.py has the rule (`np_whole_graph`) and the arguments.  On a device graph: a
        `_DeviceGraph` built on the device from the CSRs (csrc/hgt_graph_view.hip; nothing is copied to the host, an unfiltered view
        reads nothing back, a filtered one reads rel_ptr and a flag word once), with `.sorted`, `.plan` (plan=True: built by
        `GraphPlan.from_sorted` and registered, so the first layer's lookup hits), `.rows(type, ids=None)` and `.type_rows(type)`;
        node_feature is the types' resident feature matrices concatenated in type order (ValueError: a type with nodes and no
        features, or differing widths).  On a host-only graph: the numpy definition's tuple as CPU tensors.
        `gnn(*view[:5])[view.type_rows("paper")]` are the embeddings of all papers; `gnn(*view[:5], seeds=view.rows("paper", ids))`
        is the exact output at those nodes."""
        from .view import whole_graph
        return whole_graph(self, node_time, max_time, leave_out, self_loops, plan)

    def neighbourhood(self, seeds, n_layers, node_time=None, max_time=None, leave_out=None, self_loops=True, max_rows=None,
                      max_edges=None):
        """The exact n_layers-hop neighbourhood of `seeds` = {type name: ids} (tensor, array or list, on the device or the host; any
        order, repeats allowed; the dict's order is the order of the result rows) as a `NeighbourhoodGraph`: array for array the
        whole-graph view of the same arguments trimmed to the seeds (pyhgt_amd/neighbourhood.py has the rule, `np_neighbourhood`),
        with the rows' features already gathered.  `gnn(*nb.inputs, trim=nb)` is the exact output at the seeds -- equal to
        `gnn(*view[:5], seeds=...)` -- at a cost that follows the neighbourhood: a frontier walk over the in-edge CSRs
        (csrc/hgt_neighbourhood.hip), no launch and no allocation proportional to the graph after the first call, one host read per
        level (at most n_layers + 1).  Under grad the same call is full-neighbour mini-batch training.  max_rows / max_edges: a
        protective cap on the rows / edges reached so far, checked after every level (OverflowError names the level and the size).
        KeyError: an unknown seed type or leave_out triple.  IndexError: a seed id outside its type, a kept edge whose time
        difference is outside [0, 240).  ValueError: n_layers outside [1, HGT_TRIM_MAX_LAYERS], the view's node_time rules, feature
        widths that differ.  After any of these the next call is correct.  Calls on one graph share its resident marks: they are
        NOT reentrant (one call at a time, on one stream).  On a host-only graph: the definition's arrays as CPU tensors.

        node_time / leave_out tables are per-node arrays, so THEIR cost is of the graph's size -- once: the first call that is handed a
        table object validates it (host arrays on the host; an int64 device tensor with one host read, counted in `host_reads`),
        converts it to int32 / uint8 and keeps that device form with the graph under the object's identity (the object is held);
        every later call with the SAME object touches nothing of N.  An int32 (uint8) device tensor is taken as it is.  A table
        changed in place keeps its identity: call `forget_neighbourhood_tables()` (or pass a new object).  The caps are checked when a
        level's exact size is known; the buffers of a level are sized before that by the CSR entries of its rows -- an upper bound that
        `max_time` / `leave_out` can undercut by any factor -- so on a filtered call the caps bound the result, not the scratch of the
        level that trips them (unfiltered, the bound is exact and `max_edges` is checked before anything is allocated)."""
        from .neighbourhood import neighbourhood
        return neighbourhood(self, seeds, n_layers, node_time, max_time, leave_out, self_loops, max_rows, max_edges)

    def forget_neighbourhood_tables(self):
        """drop the resident forms of the node_time / leave_out tables `neighbourhood` keeps (after a table was changed in place)"""
        self._nb_tables.clear()

    def get_types(self):
        return list(self.types)

    def get_meta_graph(self):
        return list(self.meta)


def _host_array(f):
    """a feature matrix as float32 numpy (the features of a graph built on the device may be device tensors)"""
    return f.detach().cpu().numpy().astype(np.float32, copy=False) if isinstance(f, torch.Tensor) else np.asarray(f, dtype=np.float32)


def _seed_arrays(dgraph, inp):
    """inp = {type: [[id, time], ...]} (data.py:135-137) -> per type (ids int32, times int32), in get_types() order."""
    out = []
    for t, n in zip(dgraph.types, dgraph.n_nodes):
        a = np.asarray(inp.get(t, []), dtype=np.int64).reshape(-1, 2)
        if a.shape[0] and (a[:, 0].min() < 0 or a[:, 0].max() >= n):
            raise IndexError("pyhgt_amd: seed ids of %r outside [0, %d)" % (t, n))
        if np.unique(a[:, 0]).size != a.shape[0]:
            raise ValueError("pyhgt_amd: seed ids of %r repeat" % t)
        out.append((a[:, 0].astype(np.int32), a[:, 1].astype(np.int32)))
    unknown = set(inp) - set(dgraph.types)
    if unknown:
        raise KeyError("pyhgt_amd: seed types %r are not node types of the graph" % sorted(unknown))
    return out


def _capacities(dgraph, n_seed, depth, sn):
    """Static list capacities: sampled nodes per type <= seeds + depth * sampled_number, candidates <= sampled targets * sampled_number
    summed over the triples whose source is the type; both capped by the type's node count."""
    T = len(dgraph.types)
    reach = [any(st == t for _, st, _ in dgraph.tri_types) for t in range(T)]
    cap_s = [min(dgraph.n_nodes[t], n_seed[t] + (depth * sn if reach[t] else 0)) for t in range(T)]
    cap_c = [min(dgraph.n_nodes[t], sum(cap_s[tt] * sn for tt, st, _ in dgraph.tri_types if st == t)) for t in range(T)]
    return cap_s, cap_c


def _check_args(dgraph, sampled_depth, sampled_number):
    if sampled_depth < 0 or not 1 <= sampled_number <= _lib.HGT_SAMPLER_MAX_NUMBER:
        raise ValueError("pyhgt_amd: sampled_depth >= 0 and 1 <= sampled_number <= %d" % _lib.HGT_SAMPLER_MAX_NUMBER)


def _mask_table(dgraph, mask):
    """mask = {(target type, source type, relation): (tgt_below, src_below)} -> int32 [n_triples, 2] in the order of dgraph.triples, or
    None for None / {} (the unmasked call).  A table that went through here passes unchanged."""
    if isinstance(mask, np.ndarray):
        return mask
    if not mask:
        return None
    table = np.zeros((len(dgraph.triples), 2), np.int32)
    where = {tri: m for m, tri in enumerate(dgraph.triples)}
    for tri, pair in mask.items():
        if tuple(tri) not in where:
            raise KeyError("pyhgt_amd: %r is not a meta triple of the graph" % (tri,))
        tgt_below, src_below = (int(v) for v in pair)
        if tgt_below < 0 or src_below < 0:
            raise ValueError("pyhgt_amd: mask thresholds of %r are negative" % (tri,))
        table[where[tuple(tri)]] = (min(tgt_below, 2 ** 31 - 1), min(src_below, 2 ** 31 - 1))
    return table


def seed_edge_mask(dgraph, relations, node_type, below):
    """The mask that takes the edges of `relations` at the first `below` nodes of `node_type` out of a batch: for every meta triple
    whose relation is in `relations`, tgt_below = below if its target type is node_type and src_below = below if its source type is.
    seed_edge_mask(dg, ["PF_in_L2", "rev_PF_in_L2"], "paper", batch_size) is the masking step of the reference's
    node_classification_sample (train_paper_field.py:109-122) when the papers to classify are the first seeds."""
    relations, below = set(relations), int(below)
    if node_type not in dgraph.types:
        raise KeyError("pyhgt_amd: %r is not a node type of the graph" % (node_type,))
    if below < 0:
        raise ValueError("pyhgt_amd: mask thresholds are not negative")
    unknown = relations - {rel for _, _, rel in dgraph.triples}
    if unknown:
        raise KeyError("pyhgt_amd: %r are not relations of the graph" % sorted(unknown))
    return {(tt, st, rel): (below if tt == node_type else 0, below if st == node_type else 0)
            for tt, st, rel in dgraph.triples if rel in relations}


# ---------------------------------------------------------------------------------------------------------------- numpy rule
def _flat_rows(indptr, targets):
    """positions of all neighbours of `targets` (in order) -> (flat positions, row index of each, degree per row)"""
    beg = indptr[targets].astype(np.int64)
    deg = indptr[np.asarray(targets) + 1].astype(np.int64) - beg
    total = int(deg.sum())
    row = np.repeat(np.arange(len(targets)), deg)
    first = np.cumsum(deg) - deg
    pos = np.arange(total) - first[row]
    return beg[row] + pos, row, deg, pos


def np_budget_contributions(csr, m, targets, target_times, step, sn, max_time, seed, src_serial):
    """data.py:112-130 for the rows (triple m, target) of one call: -> (source ids, score terms uint64, stamps uint64) of the
    surviving neighbours, one entry per contribution."""
    indptr, src, time = csr
    targets = np.asarray(targets, dtype=np.int64)
    flat, row, deg, pos = _flat_rows(indptr, targets)
    keep = np.ones(flat.size, bool)
    first = np.cumsum(deg) - deg
    for r in np.nonzero(deg > sn)[0]:                       # rows that draw: the sn smallest (word, position)
        p = np.arange(deg[r])
        words = philox4x32_10(p, targets[r], step, _SUBSET_TAG + m, seed)[0]
        drop = np.lexsort((p, words))[sn:]
        keep[first[r] + drop] = False
    flat, row = flat[keep], row[keep]
    ln = np.minimum(deg, sn)[row]
    add = (((1 << 33) + ln) // (2 * ln)).astype(np.uint64)
    s, tm = src[flat].astype(np.int64), time[flat].astype(np.int64)
    tm = np.where(tm == TIME_NONE, np.asarray(target_times, dtype=np.int64)[row], tm)
    ok = src_serial[s] < 0
    if max_time is not None:
        ok &= tm <= max_time
    return s[ok], add[ok], (np.uint64(step) << np.uint64(32)) | _bias(tm[ok])


def np_apply_budget(score, stamp, s, add, st):
    """the atomics of add_budget: -> ids touched for the first time (ascending)"""
    fresh = np.unique(s[score[s] == 0])
    np.add.at(score, s, add)
    np.maximum.at(stamp, s, st)
    return fresh


def np_select_keys(ids, score, t, step, seed):
    """float64 selection keys of the candidates `ids` of type t"""
    word = philox4x32_10(np.asarray(ids, dtype=np.int64), t, step, _SELECT_TAG, seed)[0]
    u = ((word >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    s = score[ids].astype(np.float64) * 2.0 ** -32
    return -np.log(u) / (s * s)


def np_select(ids, score, t, step, seed, sn):
    """-> the chosen candidates in serial order"""
    ids = np.asarray(ids, dtype=np.int64)
    keys = np_select_keys(ids, score, t, step, seed)
    return ids[np.lexsort((ids, keys))[:min(sn, ids.size)]]


def np_induce(dgraph, sampled, times, serial, mask=None):
    """data.py:183-209 + 240-250 over the node lists `sampled[t]` (ids in serial order), their times and the serial arrays:
    -> (src, dst, edge_time, rel_ptr, type_off) in the sorted int32 form.  mask (the dict of the module docstring): an edge of triple m
    from the source of serial `ser` to the target of serial `row` is left out iff row < tgt_below[m] or ser < src_below[m]."""
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    table = _mask_table(dgraph, mask)
    type_off = np.concatenate([[0], np.cumsum([len(sampled[t]) for t in range(T)])]).astype(np.int64)
    srcs, dsts, tms, per_rel = [], [], [], np.zeros(R, np.int64)
    for m, ((tt, st, rel), (indptr, src, _)) in enumerate(zip(dgraph.tri_types, dgraph.csr)):
        flat, row, _, _ = _flat_rows(indptr, np.asarray(sampled[tt], dtype=np.int64))
        s = src[flat].astype(np.int64)
        ser = serial[st][s].astype(np.int64)
        ok = ser >= 0
        if table is not None:
            ok &= (row >= table[m, 0]) & (ser >= table[m, 1])
        srcs.append(ser[ok] + type_off[st])
        dsts.append(row[ok] + type_off[tt])
        tms.append(np.asarray(times[tt], dtype=np.int64)[row[ok]] - np.asarray(times[st], dtype=np.int64)[ser[ok]] + 120)
        per_rel[rel] += int(ok.sum())
    n = int(type_off[-1])
    srcs.append(np.arange(n)); dsts.append(np.arange(n)); tms.append(np.full(n, 120, np.int64))
    per_rel[R - 1] += n
    rel_ptr = np.concatenate([[0], np.cumsum(per_rel)])
    cat = lambda a: np.concatenate(a).astype(np.int32)
    return cat(srcs), cat(dsts), cat(tms), rel_ptr.astype(np.int32), type_off.astype(np.int32)


class _Seeds:
    """what a sampled result knows about its seeds: `.n_seed` = {type: count}; the seeds of a type are its first nodes"""
    n_seed = None

    def seed_rows(self, node_type):
        """global rows (int64 tensor on the result's device) of the seeds of `node_type`, in the order given: `x_ids` of the scripts"""
        return self[5][node_type][0] + torch.arange(self.n_seed[node_type], dtype=torch.int64, device=self[1].device)


class _HostGraph(_Seeds, tuple):
    """Result of sample_subgraph_host: the 7-tuple of to_torch (CPU tensors) with `.sorted` (numpy), `.indxs`, `.times`, `.n_seed`."""
    sorted = None
    indxs = None
    times = None
    plan = None


class _SampledDeviceGraph(_Seeds, _DeviceGraph):
    """Result of sample_subgraph_device: a `_DeviceGraph` with `.indxs`, `.times` and `.n_seed`."""


def candidate_pairs(g, name_label, target_type="paper", candidate_type="author"):
    """The keys of the author-disambiguation script (OAG/train_author_disambiguation.py:280-289) for a sampled piece `g` whose seeds
    are the papers and the candidate authors: `name_label[i]` = the serials among the `candidate_type` seeds of paper seed i's
    candidates, the true one first.  -> (paper_key, author_key, sizes): two int64 row tensors on g's device, one entry per (paper,
    candidate) pair in order -- `node_rep[paper_key]`, `node_rep[author_key]` feed Matcher(pair=True) -- and `sizes` (numpy int64, the
    script's `key_size`).  One host array of serials goes to the device; the rows are gathered from `seed_rows` there."""
    if len(name_label) != g.n_seed[target_type]:
        raise ValueError("pyhgt_amd: %d candidate lists for %d %s seeds" % (len(name_label), g.n_seed[target_type], target_type))
    sizes = np.fromiter((len(c) for c in name_label), dtype=np.int64, count=len(name_label))
    flat = np.fromiter((a for c in name_label for a in c), dtype=np.int64, count=int(sizes.sum()))
    if flat.size and (flat.min() < 0 or flat.max() >= g.n_seed[candidate_type]):
        raise IndexError("pyhgt_amd: candidate serials outside [0, %d)" % g.n_seed[candidate_type])
    targets, candidates = g.seed_rows(target_type), g.seed_rows(candidate_type)
    dev = targets.device
    paper_key = torch.repeat_interleave(targets, torch.from_numpy(sizes).to(dev), output_size=int(flat.size))
    return paper_key, candidates[torch.from_numpy(flat).to(dev)], sizes


def _wire_tuple(cls, dgraph, feat, n_per_type, src, dst, etime, rel_ptr, type_off):
    """the reference's int64 tensors, derived as to_device_graph derives them"""
    dev = src.device
    T, R = len(dgraph.types), len(dgraph.edge_dict)
    N, E = int(sum(n_per_type)), int(src.numel())
    node_type = torch.repeat_interleave(torch.arange(T, device=dev), torch.as_tensor(n_per_type, dtype=torch.int64, device=dev), output_size=N)
    edge_type = torch.repeat_interleave(torch.arange(R, device=dev), rel_ptr.long().diff(), output_size=E)
    edge_index = torch.stack([src.long(), dst.long()], dim=1).t()
    node_dict, n = {}, 0
    for i, t in enumerate(dgraph.types):
        node_dict[t] = [n, i]
        n += int(n_per_type[i])
    return cls((feat, node_type, etime.long(), edge_index, edge_type, node_dict, dict(dgraph.edge_dict)))


def sample_subgraph_host(dgraph, max_time, sampled_depth, sampled_number, inp, seed, trace=None, mask=None):
    """numpy sibling of `sample_subgraph_device`: the same definition on the host copy of the graph.  Returns a `_HostGraph`.
    trace: a list that receives, per select step, (type index, step, candidate ids, their float64 keys) -- what decides whether a
    fp32 key order can differ from this one (tests).  mask: the edges to leave out of the induced graph (module docstring)."""
    _check_args(dgraph, sampled_depth, sampled_number)
    table = _mask_table(dgraph, mask)
    T, sn = len(dgraph.types), int(sampled_number)
    seeds = _seed_arrays(dgraph, inp)
    if dgraph._host_state is None:
        dgraph._host_state = ([np.zeros(n, np.uint64) for n in dgraph.n_nodes], [np.zeros(n, np.uint64) for n in dgraph.n_nodes],
                              [np.full(n, -1, np.int32) for n in dgraph.n_nodes])
    score, stamp, serial = dgraph._host_state
    sampled = [np.zeros(0, np.int64) for _ in range(T)]
    cand = [np.zeros(0, np.int64) for _ in range(T)]

    def add_budget(t, new, step):
        times = _stamp_time(stamp[t][new])
        for m, (tt, st, _) in enumerate(dgraph.tri_types):
            if tt != t or new.size == 0:
                continue
            s, add, stp = np_budget_contributions(dgraph.csr[m], m, new, times, step, sn, max_time, seed, serial[st])
            cand[st] = np.concatenate([cand[st], np_apply_budget(score[st], stamp[st], s, add, stp)])

    try:
        for t, (ids, tms) in enumerate(seeds):
            sampled[t] = ids.astype(np.int64)
            serial[t][ids] = np.arange(ids.size, dtype=np.int32)
            stamp[t][ids] = (np.uint64(t) << np.uint64(32)) | _bias(tms)
        for t in range(T):
            add_budget(t, sampled[t], t)
        for layer in range(sampled_depth):
            for t in range(T):
                step = T * (1 + layer) + t
                keys = np_select_keys(cand[t], score[t], t, step, seed)
                new = cand[t][np.lexsort((cand[t], keys))[:min(sn, cand[t].size)]]      # np_select, with the keys kept
                if trace is not None:
                    trace.append((t, step, cand[t].copy(), keys))
                serial[t][new] = np.arange(sampled[t].size, sampled[t].size + new.size, dtype=np.int32)
                sampled[t] = np.concatenate([sampled[t], new])
                cand[t] = np.setdiff1d(cand[t], new)
                add_budget(t, new, step)
        times = [_stamp_time(stamp[t][sampled[t]]) for t in range(T)]
        src, dst, etime, rel_ptr, type_off = np_induce(dgraph, sampled, times, serial, table)
    finally:                                                 # walk the lists the call touched
        for t in range(T):
            for ids in (sampled[t], cand[t]):
                score[t][ids], stamp[t][ids], serial[t][ids] = 0, 0, -1
    width = max([f.shape[1] for f in (dgraph.features_host or []) if f is not None] + [0])
    feat = [np.zeros((0, width), np.float32) if dgraph.features_host is None or dgraph.features_host[t] is None or sampled[t].size == 0
            else _host_array(dgraph.features_host[t])[sampled[t]] for t in range(T)]
    feat = np.concatenate(feat, axis=0) if width else np.zeros((int(type_off[-1]), 0), np.float32)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = _wire_tuple(_HostGraph, dgraph, tt(feat), [sampled[t].size for t in range(T)], tt(src), tt(dst), tt(etime), tt(rel_ptr), tt(type_off))
    out.sorted = (src, dst, etime, rel_ptr, type_off)
    out.indxs = {name: sampled[t] for t, name in enumerate(dgraph.types)}
    out.times = {name: times[t] for t, name in enumerate(dgraph.types)}
    out.n_seed = {name: int(seeds[t][0].size) for t, name in enumerate(dgraph.types)}
    return out


# ---------------------------------------------------------------------------------------------------------------- device
def _triple_table(dgraph):
    """the resident CSRs as the C table of meta triples"""
    ptr = _lib.ptr
    triples_c = (_lib.HgtSamplerTriple * max(len(dgraph.triples), 1))()
    for m, ((tt, st, rel), (ip, src, tm)) in enumerate(zip(dgraph.tri_types, dgraph.csr_dev)):
        triples_c[m] = _lib.HgtSamplerTriple(ip.data_ptr(), ptr(src), ptr(tm), tt, st, rel, 0)
    return triples_c


def _scratch_entries(lib, dgraph, types_c, triples_c, n_seed, sn):
    """entries of rowoff / hub for one batch: the row slots of the induction or the rows of the largest add_budget call, + 1"""
    T, slots = len(dgraph.types), C.c_int64()
    _lib.check(lib.hgt_sampler_induce_slots(types_c, T, triples_c, len(dgraph.triples), C.byref(slots)), "hgt_sampler_induce_slots")
    into = [sum(1 for tt, _, _ in dgraph.tri_types if tt == t) for t in range(T)]
    rows = max([max(n_seed[t], sn) * into[t] for t in range(T)] + [0])       # add_budget: max_new x triples into the type
    return max(int(slots.value), rows) + 1


def _masks_c(table, M):
    masks_c = (_lib.HgtSamplerMask * max(M, 1))()
    for m in range(M):
        masks_c[m] = _lib.HgtSamplerMask(int(table[m, 0]), int(table[m, 1]))
    return masks_c


def _need_gpu(dgraph, call):
    if dgraph.device is None or dgraph.device.type != "cuda":
        raise RuntimeError("pyhgt_amd: %s_device needs a DeviceHeteroGraph on a GPU (no CPU fallback; the host sibling is %s_host)"
                           % (call, call))


class _SamplerState:
    """The device state of one (seed counts, depth, sampled_number) shape of call and the step-level calls on it (one method per C
    entry point), written once for the single call and for n_batch replicas drawn at once.  `lead` is the leading shape of every
    array: () for `DeviceSamplerState`, (n_batch,) for `BatchedDeviceSamplerState`, where replica b of every launch is blockIdx.y = b,
    replica b's arrays are base + b * stride and the strides are the fields of the one table the kernels get (n_nodes, cap_sampled,
    cap_cand).  The two specialisations name the entry points (`_suffix`), the public call that error messages speak of (`_public`)
    and the attributes of the graph that hold their per-node arrays, their cache and (`dirty`) their flag.  `draw` strings the steps
    together for the public calls; the tests call them one by one."""

    def __init__(self, dgraph, n_seed, depth, sn, lead):
        _need_gpu(dgraph, self._public)
        if lead and not 1 <= lead[0] <= _lib.HGT_SAMPLER_MAX_BATCH:
            raise ValueError("pyhgt_amd: 1 <= n_batch <= %d" % _lib.HGT_SAMPLER_MAX_BATCH)
        self.g, self.dev, self.sn, self.depth = dgraph, dgraph.device, int(sn), int(depth)
        self.lead = lead = tuple(int(b) for b in lead)
        self.B = B = lead[0] if lead else 1
        self.lib = _lib.load()
        T, M, dev = len(dgraph.types), len(dgraph.triples), self.dev
        self.T, self.M, self.R = T, M, len(dgraph.edge_dict)
        self.cap_s, self.cap_c = _capacities(dgraph, n_seed, depth, sn)
        # The per-node arrays (score / stamp / serial over every node of every type, 20 bytes x nodes x B) live on the graph, shared by
        # every shape of call; the batched set is apart from the single call's and sized for the largest n_batch seen.  New arrays are
        # clean, and the cached states point into the arrays that go.
        nodes = getattr(dgraph, self._nodes)
        if nodes is None or (lead and nodes[0][0].size(0) < B):
            getattr(dgraph, self._cache).clear()
            nodes = ([torch.zeros(*lead, n, dtype=torch.int64, device=dev) for n in dgraph.n_nodes],
                     [torch.zeros(*lead, n, dtype=torch.int64, device=dev) for n in dgraph.n_nodes],
                     [torch.full((*lead, n), -1, dtype=torch.int32, device=dev) for n in dgraph.n_nodes])
            setattr(dgraph, self._nodes, nodes)
            self.dirty = False
        self.score, self.stamp, self.serial = nodes
        i32 = dict(dtype=torch.int32, device=dev)
        self.sampled = [torch.zeros(*lead, c, **i32) for c in self.cap_s]
        self.cand = [torch.zeros(*lead, c, **i32) for c in self.cap_c]
        self.counts = torch.zeros(*lead, T, 4, **i32)
        ptr = _lib.ptr
        self.types_c = (_lib.HgtSamplerType * T)()           # the table of replica 0; the batched kernels shift it by b strides
        for t in range(T):
            self.types_c[t] = _lib.HgtSamplerType(ptr(self.score[t]), ptr(self.stamp[t]), ptr(self.serial[t]), ptr(self.sampled[t]),
                                                  ptr(self.cand[t]), self.counts.data_ptr() + 16 * t, dgraph.n_nodes[t], self.cap_s[t],
                                                  self.cap_c[t], 0)
        self.triples_c = _triple_table(dgraph)
        self.n_entries = _scratch_entries(self.lib, dgraph, self.types_c, self.triples_c, n_seed, sn)      # per replica
        self.rowoff, self.hub = torch.zeros(*lead, self.n_entries, **i32), torch.zeros(B * self.n_entries, **i32)
        self.n_tmp = max(self.cap_c + [1])
        self.keys = torch.zeros(*lead, self.n_tmp, dtype=torch.int64, device=dev)
        self.tmp = torch.zeros(*lead, self.n_tmp, **i32)
        self.type_off, self.rel_ptr = torch.zeros(*lead, T + 1, **i32), torch.zeros(*lead, self.R + 1, **i32)
        self.sizes = torch.zeros(*lead, T + M + 2, **i32)
        self.fill_extra = ()                                 # batched: sizes and the offsets the fill pass writes, [2 * (B + 1)]
        if lead:
            self.offs = torch.zeros(2 * (B + 1), **i32)
            self.fill_extra = (self.sizes.data_ptr(), self.offs.data_ptr())

    # The entry points are bound when the library is set, not looked up by name on every call.  The tests put a counting library
    # into `lib` after construction; setting it binds again.
    @property
    def lib(self):
        return self._library

    @lib.setter
    def lib(self, lib):
        self._library = lib
        entry = lambda step: getattr(lib, "hgt_sampler_" + step + self._suffix)
        self.c_seed, self.c_add_budget, self.c_select, self.c_reset = entry("seed"), entry("add_budget"), entry("select"), entry("reset")
        self.c_induce = {False: (entry("induce_count"), entry("induce_fill"), "hgt_sampler_induce" + self._suffix),
                         True: (entry("induce_count_masked"), entry("induce_fill_masked"), "hgt_sampler_induce_masked" + self._suffix)}

    def _stream(self):
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _seeds_c(self, seeds):
        """the Philox seeds of a batched call as the HOST array the entry points take"""
        if len(seeds) != self.B:
            raise ValueError("pyhgt_amd: %d Philox seeds for %d replicas" % (len(seeds), self.B))
        return (C.c_uint64 * self.B)(*[int(s) & (2 ** 64 - 1) for s in seeds])

    def seed_nodes(self, t, ids, times, step):
        """ids, times: [n], batched [n_batch, n]"""
        ids, times = (np.ascontiguousarray(a, dtype=np.int32) for a in (ids, times))
        if self.lead and (ids.ndim != 2 or ids.shape[0] != self.B or times.shape != ids.shape):
            raise ValueError("pyhgt_amd: seed ids and times must be [%d, n]" % self.B)
        n = ids.shape[-1]
        ids, times = (torch.from_numpy(a).to(self.dev) for a in (ids, times))
        self.dirty = True
        _lib.check(self.c_seed(self.types_c, self.T, *self.lead, t, ids.data_ptr() if n else None, times.data_ptr() if n else None, n, step,
                               self._stream()), "hgt_sampler_seed" + self._suffix)
        ids.record_stream(torch.cuda.current_stream(self.dev))
        times.record_stream(torch.cuda.current_stream(self.dev))

    def add_budget(self, t, step, max_new, max_time, seed):
        """seed: the Philox seed, batched the n_batch seeds"""
        self.dirty = True
        key = self._seeds_c(seed) if self.lead else seed & (2 ** 64 - 1)
        _lib.check(self.c_add_budget(self.types_c, self.T, self.triples_c, self.M, *self.lead, t, step, self.sn, max_new,
                                     0 if max_time is None else 1, 0 if max_time is None else int(max_time), key, self.hub.data_ptr(),
                                     self.n_entries, self._stream()), "hgt_sampler_add_budget" + self._suffix)

    def select(self, t, step, seed):
        self.dirty = True
        key = self._seeds_c(seed) if self.lead else seed & (2 ** 64 - 1)
        _lib.check(self.c_select(self.types_c, self.T, *self.lead, t, step, self.sn, key, self.keys.data_ptr(), self.tmp.data_ptr(),
                                 self.n_tmp, self._stream()), "hgt_sampler_select" + self._suffix)

    def induce(self, mask=None):
        """count pass, the one host read of the call (sizes [T + M + 2] per replica), fill pass -> (src, dst, edge_time, rel_ptr,
        type_off, node_time, node_id, nodes per type).  Batched: the buffers hold the replicas one after the other with indices local
        to each piece, rel_ptr is [B, R + 1], type_off [B, T + 1], nodes per type [B][T], and the node offsets [B + 1] and the edge
        offsets [B + 1] follow.  mask (dict or the table of _mask_table): the masked entry points, the same launches with the
        thresholds as one more argument; None or {}: the unmasked ones."""
        T, M = self.T, self.M
        table = _mask_table(self.g, mask)
        count, fill, what = self.c_induce[table is not None]
        tail = () if table is None else (_masks_c(table, M),)
        head = (self.types_c, T, self.triples_c, M, *self.lead, self.R, self.rowoff.data_ptr(), self.hub.data_ptr(), self.n_entries,
                self.type_off.data_ptr())
        _lib.check(count(*head, self.rel_ptr.data_ptr(), self.sizes.data_ptr(), *tail, self._stream()), what + " (count)")
        sizes = self.sizes.cpu().numpy().reshape(self.B, T + M + 2)      # the host synchronisation of the call
        if sizes[:, T + M].any():
            raise RuntimeError("pyhgt_amd: a sampler list overflowed its static capacity or a seed id was out of range")
        n_per_type = [[int(v) for v in row[:T]] for row in sizes]
        nodes = [sum(row) for row in n_per_type]
        edges = [n + int(row[T + M + 1]) for n, row in zip(nodes, sizes)]
        N, E = sum(nodes), sum(edges)
        i32 = dict(dtype=torch.int32, device=self.dev)
        src, dst, etime = torch.empty(E, **i32), torch.empty(E, **i32), torch.empty(E, **i32)
        node_time, node_id = torch.empty(N, **i32), torch.empty(N, **i32)
        ptr = _lib.ptr
        _lib.check(fill(*head, *self.fill_extra, N, E, ptr(src), ptr(dst), ptr(etime), ptr(node_time), ptr(node_id), *tail, self._stream()),
                   what + " (fill)")
        out = (src, dst, etime, self.rel_ptr.clone(), self.type_off.clone(), node_time, node_id)
        if not self.lead:
            return out + (n_per_type[0],)
        prefix = lambda v: np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
        return out + (n_per_type, prefix(nodes), prefix(edges))

    def reset(self):
        _lib.check(self.c_reset(self.types_c, self.T, *self.lead, self._stream()), "hgt_sampler_reset" + self._suffix)
        self.dirty = False

    def clear(self):
        """full clear of the per-node arrays (all the graph holds of this set, not only this state's replicas): after a call that
        failed half way.  The counters of every cached state go with them: the state that failed is not the one that finds the graph
        dirty when the next call has another shape."""
        for a in self.score + self.stamp:
            a.zero_()
        for a in self.serial:
            a.fill_(-1)
        for st in [self] + list(getattr(self.g, self._cache).values()):
            st.counts.zero_()
        self.dirty = False

    def draw(self, seeds, max_time, seed, table):
        """one whole draw up to the induced graph: seeds = per type (ids, times) in the form of seed_nodes -> what induce returns"""
        T = self.T
        if self.dirty:
            self.clear()
        for t, (ids, tms) in enumerate(seeds):
            if ids.shape[-1]:
                self.seed_nodes(t, ids, tms, t)
        for t, (ids, _) in enumerate(seeds):
            if ids.shape[-1]:
                self.add_budget(t, t, ids.shape[-1], max_time, seed)
        for layer in range(self.depth):
            for t in range(T):
                if self.cap_c[t] == 0:                       # nothing can ever be a candidate of this type
                    continue
                step = T * (1 + layer) + t
                self.select(t, step, seed)
                self.add_budget(t, step, self.sn, max_time, seed)
        return self.induce(table)

    def snapshot(self):
        """host copies of the state (tests): score / stamp as uint64, serial, the two lists cut to their counts, as one dict; batched:
        a list of such dicts, one per replica"""
        rows = (lambda a: a) if self.lead else (lambda a: a[None])
        counts = rows(self.counts.cpu().numpy())
        score, stamp = ([rows(a.cpu().numpy().view(np.uint64)) for a in v] for v in (self.score, self.stamp))
        serial, sampled, cand = ([rows(a.cpu().numpy()) for a in v] for v in (self.serial, self.sampled, self.cand))
        out = [dict(score=[a[b] for a in score], stamp=[a[b] for a in stamp], serial=[a[b] for a in serial],
                    sampled=[a[b, :counts[b, t, 0]].astype(np.int64) for t, a in enumerate(sampled)],
                    cand=[a[b, :counts[b, t, 2]].astype(np.int64) for t, a in enumerate(cand)], counts=counts[b]) for b in range(self.B)]
        return out if self.lead else out[0]


class DeviceSamplerState(_SamplerState):
    """the state of `sample_subgraph_device`: one draw, 1-D arrays per type, counts [T, 4]"""
    _suffix, _public, _nodes, _cache = "", "sample_subgraph", "_dev_nodes", "_dev_state"

    def __init__(self, dgraph, n_seed, depth, sn):
        super().__init__(dgraph, n_seed, depth, sn, ())

    # Clean or dirty is a fact about the per-node arrays, which every shape of call shares: it lives on the graph.  A state that
    # starts on a graph another state left dirty (a call that raised half way, a state evicted from the cache) sees it.
    @property
    def dirty(self):
        return self.g._dev_dirty

    @dirty.setter
    def dirty(self, value):
        self.g._dev_dirty = bool(value)


class BatchedDeviceSamplerState(_SamplerState):
    """the state of `sample_subgraphs_device`: n_batch replicas, every array one [n_batch, .] tensor, counts [n_batch, T, 4].  The
    lists, keys and induction scratch (a few hundred KB per replica at the training shapes) belong to the state."""
    _suffix, _public, _nodes, _cache = "_batched", "sample_subgraphs", "_batch_nodes", "_batch_state"

    def __init__(self, dgraph, n_seed, depth, sn, n_batch):
        super().__init__(dgraph, n_seed, depth, sn, (n_batch,))

    # the state rule of the single call with a flag of its own: the batched per-node arrays are another set of arrays
    @property
    def dirty(self):
        return self.g._batch_dirty

    @dirty.setter
    def dirty(self, value):
        self.g._batch_dirty = bool(value)

    def gather_features(self, type_off, node_id, n_per_type, width):
        """the feature rows of every replica's nodes in one launch: float32 [nodes of the call, width].  self.offs still holds the
        node offsets the fill pass wrote.  A type with rows and no matrix is an error of the caller, found here before the launch."""
        N = int(node_id.numel())
        feats = self.g.features
        for t in range(self.T):
            if width and feats[t] is None and any(row[t] for row in n_per_type):
                raise ValueError("pyhgt_amd: no feature matrix for node type %r" % self.g.types[t])
        out = torch.empty(N, width, dtype=torch.float32, device=self.dev)
        mats = (C.c_void_p * self.T)(*[None if f is None or f.numel() == 0 else f.data_ptr() for f in feats])
        rows = (C.c_int32 * self.T)(*[0 if f is None else int(f.size(0)) for f in feats])
        _lib.check(self.lib.hgt_sampler_gather_features(mats, rows, self.T, self.B, width, type_off.data_ptr(), self.offs.data_ptr(),
                                                        node_id.data_ptr() if N else None, N, out.data_ptr() if out.numel() else None,
                                                        self._stream()), "hgt_sampler_gather_features")
        return out


def _cached_state(cls, dgraph, n_seed, depth, sn, *n_batch):
    """the state of this shape of call from the graph's cache of `cls` states"""
    cache = getattr(dgraph, cls._cache)
    key = (tuple(n_seed), int(depth), int(sn)) + tuple(int(b) for b in n_batch)
    st = cache.get(key)
    if st is None:
        if len(cache) >= 4:                                  # a loop uses one or two shapes of call; do not hoard lists
            cache.clear()
        st = cls(dgraph, n_seed, depth, sn, *n_batch)
        cache[key] = st                                      # after the constructor: a larger n_batch empties the cache in there
    return st


def _device_state(dgraph, n_seed, depth, sn):
    return _cached_state(DeviceSamplerState, dgraph, n_seed, depth, sn)


def _batched_state(dgraph, n_seed, depth, sn, n_batch):
    return _cached_state(BatchedDeviceSamplerState, dgraph, n_seed, depth, sn, n_batch)


def _feature_width(dgraph):
    widths = sorted({f.size(1) for f in dgraph.features if f is not None and f.size(0) > 0})
    if len(widths) > 1:
        raise ValueError("pyhgt_amd: feature matrices of different widths: %r" % (widths,))
    return widths[0] if widths else 0


def _call_table(dgraph, call, mask):
    """the front of both public calls behind their seeds: the mask table, then what the graph must have"""
    table = _mask_table(dgraph, mask)
    _need_gpu(dgraph, call)
    if dgraph.features is None:
        raise ValueError("pyhgt_amd: the DeviceHeteroGraph carries no features")
    return table


def sample_subgraph_device(dgraph, max_time, sampled_depth, sampled_number, inp, seed, plan=True, mask=None):
    """Sibling of `sample_subgraph` + `to_torch` (data.py:87-256) on the device: seeds `inp = {type: [[id, time], ...]}` -> the
    `_DeviceGraph` 7-tuple (node_feature, node_type, edge_time, edge_index, edge_type, node_dict, edge_dict) with `.sorted`, `.plan`
    (plan=False: none, for pieces that will only be stacked), `.indxs` = {type: original ids, int64 device tensor} and `.times`.
    max_time=None: no time filter (the ogbn-mag variant).  Kernel launches are enqueued for seeds and every (layer, type) without a host
    synchronisation; the single device->host read is the sizes of the result.  The result goes straight into `stack_device_graphs`.
    mask = {(target type, source type, relation): (tgt_below, src_below)} leaves edges out of the induced graph (module docstring;
    `seed_edge_mask` builds the one of a task batch) inside the induction kernels: no further launch, no further host read.  `.n_seed`
    and `.seed_rows(type)` name the seeds' rows in the result."""
    _check_args(dgraph, sampled_depth, sampled_number)
    seeds = _seed_arrays(dgraph, inp)
    table = _call_table(dgraph, "sample_subgraph", mask)
    T = len(dgraph.types)
    st = _device_state(dgraph, [ids.size for ids, _ in seeds], sampled_depth, sampled_number)
    dev = st.dev
    with torch.cuda.device(dev):
        src, dst, etime, rel_ptr, type_off, node_time, node_id, n_per_type = st.draw(seeds, max_time, int(seed), table)
        width = _feature_width(dgraph)
        feat = torch.empty(sum(n_per_type), width, dtype=torch.float32, device=dev)
        off, stream = 0, torch.cuda.current_stream(dev).cuda_stream
        for t, n in enumerate(n_per_type):
            if n and width:
                if dgraph.features[t] is None:
                    raise ValueError("pyhgt_amd: no feature matrix for node type %r" % dgraph.types[t])
                _lib.check(st.lib.hgt_gather_rows(dgraph.features[t].data_ptr(), width, st.sampled[t].data_ptr(), n, width,
                                                  feat[off:].data_ptr(), stream), "hgt_gather_rows")
            off += n
        st.reset()
        out = _wire_tuple(_SampledDeviceGraph, dgraph, feat, n_per_type, src, dst, etime, rel_ptr, type_off)
        out.sorted = (src, dst, etime, rel_ptr, type_off)
        ids64, offs = node_id.long(), np.concatenate([[0], np.cumsum(n_per_type)])
        out.indxs = {name: ids64[offs[t]:offs[t + 1]] for t, name in enumerate(dgraph.types)}
        out.times = {name: node_time[offs[t]:offs[t + 1]] for t, name in enumerate(dgraph.types)}
        out.n_seed = {name: int(seeds[t][0].size) for t, name in enumerate(dgraph.types)}
        if plan:
            out.plan = GraphPlan.from_sorted(out[1], out[3], out[4], out[2], src, dst, etime, rel_ptr, type_off, T, st.R)
            GraphPlan.register(out.plan, out[1], out[3], out[4], out[2], T, st.R)
    return out


# ---------------------------------------------------------------------------------------------------------------- batched calls
def _batch_args(dgraph, inps, seeds):
    """-> (per replica the seed arrays of _seed_arrays, Philox seeds); every replica has the same number of seeds per type"""
    inps, seeds = list(inps), [int(s) for s in seeds]
    if not 1 <= len(inps) <= _lib.HGT_SAMPLER_MAX_BATCH:
        raise ValueError("pyhgt_amd: 1 <= number of batches <= %d, got %d" % (_lib.HGT_SAMPLER_MAX_BATCH, len(inps)))
    if len(seeds) != len(inps):
        raise ValueError("pyhgt_amd: %d Philox seeds for %d batches" % (len(seeds), len(inps)))
    arrays = [_seed_arrays(dgraph, inp) for inp in inps]
    shape = [ids.size for ids, _ in arrays[0]]
    for b, a in enumerate(arrays):
        if [ids.size for ids, _ in a] != shape:
            raise ValueError("pyhgt_amd: batch %d has %r seeds per type, batch 0 has %r (a short last batch goes through the single call)"
                             % (b, [ids.size for ids, _ in a], shape))
    return arrays, seeds


def sample_subgraphs_host(dgraph, max_time, sampled_depth, sampled_number, inps, seeds, mask=None):
    """The definition of `sample_subgraphs_device`: the list of the single host calls."""
    inps, seeds = list(inps), list(seeds)
    if len(seeds) != len(inps):
        raise ValueError("pyhgt_amd: %d Philox seeds for %d batches" % (len(seeds), len(inps)))
    return [sample_subgraph_host(dgraph, max_time, sampled_depth, sampled_number, inp, seed, mask=mask) for inp, seed in zip(inps, seeds)]


def sample_subgraphs_device(dgraph, max_time, sampled_depth, sampled_number, inps, seeds, plan=True, mask=None):
    """B sub-graphs in one pass of launches: inps = B seed dicts in the form `sample_subgraph_device` takes, all with the same number of
    seeds per type (ValueError otherwise, before any launch; 1 <= B <= HGT_SAMPLER_MAX_BATCH), seeds = B Philox seeds; max_time, depth,
    sampled_number and mask are shared.  Returns a list whose element b is, bit for bit, what sample_subgraph_device(dgraph, max_time,
    sampled_depth, sampled_number, inps[b], seeds[b], plan=plan, mask=mask) returns (random words are keyed by what is drawn and by the
    seed, serials are ranks, the state updates are integer atomics); its tensors are slices of buffers the call allocates once.  The
    number of sampler launches is that of a single call whatever B is, and the call reads the device once (the [B, T + M + 2] sizes);
    an overflow in any replica raises the single call's RuntimeError.  The list goes straight into `stack_device_graphs`.
    Memory: 20 bytes x nodes of the graph x B for the per-node state, kept on the graph for the largest B seen."""
    _check_args(dgraph, sampled_depth, sampled_number)
    arrays, seeds = _batch_args(dgraph, inps, seeds)
    table = _call_table(dgraph, "sample_subgraphs", mask)
    T, B = len(dgraph.types), len(arrays)
    n_seed = [ids.size for ids, _ in arrays[0]]
    st = _batched_state(dgraph, n_seed, sampled_depth, sampled_number, B)
    with torch.cuda.device(st.dev):
        stacked = [tuple(np.stack([a[t][k] for a in arrays]) for k in (0, 1)) for t in range(T)]      # per type ids, times [B, n]
        src, dst, etime, rel_ptr, type_off, node_time, node_id, n_per_type, node_off, edge_off = st.draw(stacked, max_time, seeds, table)
        feat = st.gather_features(type_off, node_id, n_per_type, _feature_width(dgraph))
        st.reset()
        ids64, out = node_id.long(), []
        for b in range(B):
            n, e = slice(int(node_off[b]), int(node_off[b + 1])), slice(int(edge_off[b]), int(edge_off[b + 1]))
            srt = (src[e], dst[e], etime[e], rel_ptr[b], type_off[b])
            x = feat[n] if (n.start * feat.size(1)) % 4 == 0 else feat[n].clone()      # starts on 16 bytes, like a single call's
            piece = _wire_tuple(_SampledDeviceGraph, dgraph, x, n_per_type[b], *srt)
            piece.sorted = srt
            offs = node_off[b] + np.concatenate([[0], np.cumsum(n_per_type[b])])
            piece.indxs = {name: ids64[offs[t]:offs[t + 1]] for t, name in enumerate(dgraph.types)}
            piece.times = {name: node_time[offs[t]:offs[t + 1]] for t, name in enumerate(dgraph.types)}
            piece.n_seed = {name: int(n_seed[t]) for t, name in enumerate(dgraph.types)}
            if plan:
                piece.plan = GraphPlan.from_sorted(piece[1], piece[3], piece[4], piece[2], *piece.sorted, T, st.R)
                GraphPlan.register(piece.plan, piece[1], piece[3], piece[4], piece[2], T, st.R)
            out.append(piece)
    return out


# ---------------------------------------------------------------------------------------------------------------- task labels
# The labels of a task batch come from the label relation of the FULL graph (train_paper_field.py:133-137, train_paper_venue.py:134),
# not from the sampled one, whose label edges at the seeds the mask took out.  For a row of the triple's CSR, a neighbour qualifies iff
# it has a class column (col_of[src] >= 0) and, when a window [t_min, t_max] is given, its edge time is not None and lies inside; C is
# the set of distinct columns of the qualifying neighbours.  distribution = 1 / |C| on C (float32, the IEEE quotient), index = the
# column of the first qualifying neighbour in adjacency order (-1 without one), counts = |C|.  An id outside the target type gives a
# zero row, -1 and 0.
def _window(t_min, t_max):
    """-> (has_window, t_min, t_max) as int32 values; one open end is unbounded"""
    if t_min is None and t_max is None:
        return 0, 0, 0
    lo, hi = (-2 ** 31 if t_min is None else int(t_min)), (2 ** 31 - 1 if t_max is None else int(t_max))
    if lo > hi:
        raise ValueError("pyhgt_amd: the window [%d, %d] is empty" % (lo, hi))
    return 1, max(lo, -2 ** 31), min(hi, 2 ** 31 - 1)


def _np_qualifying(csr, col_of, ids, t_min, t_max):
    """-> (row of each qualifying neighbour in adjacency order, its column, its edge time) for the rows `ids` of one CSR"""
    indptr, src, time = csr
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    valid = np.nonzero((ids >= 0) & (ids < indptr.size - 1))[0]
    flat, row, _, _ = _flat_rows(indptr, ids[valid])
    col, tm = np.asarray(col_of, dtype=np.int64)[src[flat]], time[flat].astype(np.int64)
    ok = col >= 0
    has, lo, hi = _window(t_min, t_max)
    if has:
        ok &= (tm != TIME_NONE) & (tm >= lo) & (tm <= hi)
    return valid[row[ok]], col[ok], tm[ok]


def np_label_counts(dgraph, triple, col_of, ids, t_min=None, t_max=None):
    """|C| per row: int64 [n]"""
    ids = np.asarray(ids).reshape(-1)
    row, col, _ = _np_qualifying(dgraph.csr[dgraph.triples.index(tuple(triple))], col_of, ids, t_min, t_max)
    pairs = np.unique(np.stack([row, col], axis=1), axis=0) if row.size else np.zeros((0, 2), np.int64)
    return np.bincount(pairs[:, 0], minlength=ids.size).astype(np.int64)


def np_label_distribution(dgraph, triple, col_of, n_cols, ids, t_min=None, t_max=None):
    """`ylabel` of train_paper_field.py:133-137: float32 [n, n_cols], 1 / |C| in the columns of C"""
    ids = np.asarray(ids).reshape(-1)
    row, col, _ = _np_qualifying(dgraph.csr[dgraph.triples.index(tuple(triple))], col_of, ids, t_min, t_max)
    member = np.zeros((ids.size, int(n_cols)), bool)
    member[row, col] = True
    count = member.sum(axis=1)
    value = np.float32(1.0) / np.maximum(count, 1).astype(np.float32)
    return np.where(member, value[:, None], np.float32(0.0)).astype(np.float32)


def np_label_columns(dgraph, triple, col_of, ids, t_min=None, t_max=None, width=None):
    """C as a list: (columns int32 [n, width], count int32 [n]) -- the distinct columns of each row in ascending order, the first
    `width` of them, -1 behind; count = |C| whether it fitted or not.  width=None: the largest count (at least 1)."""
    ids = np.asarray(ids).reshape(-1)
    row, col, _ = _np_qualifying(dgraph.csr[dgraph.triples.index(tuple(triple))], col_of, ids, t_min, t_max)
    pairs = np.unique(np.stack([row, col], axis=1), axis=0) if row.size else np.zeros((0, 2), np.int64)      # sorted by (row, column)
    count = np.bincount(pairs[:, 0], minlength=ids.size).astype(np.int32)
    width = max(int(count.max()) if count.size else 0, 1) if width is None else int(width)
    if width < 1:
        raise ValueError("pyhgt_amd: width >= 1")
    place = np.arange(pairs.shape[0]) - np.concatenate([[0], np.cumsum(count)[:-1]])[pairs[:, 0]]
    columns = np.full((ids.size, width), -1, np.int32)
    keep = place < width
    columns[pairs[keep, 0], place[keep]] = pairs[keep, 1]
    return columns, count


def np_label_index(dgraph, triple, col_of, ids, t_min=None, t_max=None):
    """the class of train_paper_venue.py:159-170 + :134 (the first source in the window wins): int64 [n], -1 without one"""
    ids = np.asarray(ids).reshape(-1)
    row, col, _ = _np_qualifying(dgraph.csr[dgraph.triples.index(tuple(triple))], col_of, ids, t_min, t_max)
    out = np.full(ids.size, -1, np.int64)
    rows, first = np.unique(row, return_index=True)
    out[rows] = col[first]
    return out


class LabelSpace:
    """The classes of one task: `candidates` = the source ids of the meta triple `triple` = (target type, source type, relation) in class
    order (`cand_list` of the scripts); a target node's labels are the classes of its neighbours in that relation of the full graph.
    The id -> column map is built once and lives on the device when the graph does; there `distribution` / `index` / `counts` are one
    launch of csrc/hgt_sampler_labels.hip on the current stream without a synchronisation, and `ids` may be a device tensor (e.g.
    `g.indxs["paper"][:n]`) or a host array.  On a host graph they return what the numpy siblings `np_label_*` return, as CPU tensors."""

    def __init__(self, dgraph, triple, candidates):
        triple = tuple(triple)
        if triple not in dgraph.triples:
            raise KeyError("pyhgt_amd: %r is not a meta triple of the graph" % (triple,))
        self.g, self.triple, self.m = dgraph, triple, dgraph.triples.index(triple)
        self.n_tgt, self.n_src = (dgraph.n_nodes[t] for t in dgraph.tri_types[self.m][:2])
        cand = np.asarray(candidates, dtype=np.int64).reshape(-1)
        if cand.size and (cand.min() < 0 or cand.max() >= self.n_src):
            raise IndexError("pyhgt_amd: candidate ids outside [0, %d)" % self.n_src)
        if np.unique(cand).size != cand.size:
            raise ValueError("pyhgt_amd: candidate ids repeat")
        self.candidates, self.n_cols = cand, int(cand.size)
        self.col_of = np.full(self.n_src, -1, np.int32)
        self.col_of[cand] = np.arange(cand.size, dtype=np.int32)
        self.device = dgraph.device
        if self.device is not None:
            self.col_of_dev = torch.from_numpy(self.col_of).to(self.device)
            ip, src, tm = dgraph.csr_dev[self.m]
            ptr = _lib.ptr
            self._triple_c = _lib.HgtSamplerTriple(ip.data_ptr(), ptr(src), ptr(tm), *dgraph.tri_types[self.m], 0)

    def _device_ids(self, ids):
        ids = torch.as_tensor(ids).reshape(-1).to(self.device)
        outside = (ids < 0) | (ids >= self.n_tgt)                                # also what an int64 id would wrap to
        return torch.where(outside, torch.full_like(ids, -1), ids).to(torch.int32).contiguous()

    def _launch(self, ids, t_min, t_max, dist=None, index=None, count=None):
        has, lo, hi = _window(t_min, t_max)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().hgt_sampler_labels(C.byref(self._triple_c), self.n_tgt, self.n_src, ids.data_ptr() if ids.numel() else None,
                                                      ids.numel(), self.col_of_dev.data_ptr() if self.n_src else None, self.n_cols, has, lo, hi,
                                                      None if dist is None or not dist.numel() else dist.data_ptr(),
                                                      0 if dist is None else max(dist.stride(0), self.n_cols),
                                                      None if index is None else index.data_ptr(), None if count is None else count.data_ptr(),
                                                      torch.cuda.current_stream(self.device).cuda_stream), "hgt_sampler_labels")
            ids.record_stream(torch.cuda.current_stream(self.device))

    def distribution(self, ids, t_min=None, t_max=None, out=None):
        """float32 [n, C]: 1 / |C_r| in the columns of row r's classes (`ylabel` of the paper-field script).  out: a float32 device
        tensor [n, C] with unit column stride -- e.g. the first C columns of a wider one -- whose rows the kernel writes whole."""
        if self.device is None:
            return torch.from_numpy(np_label_distribution(self.g, self.triple, self.col_of, self.n_cols, ids, t_min, t_max))
        ids = self._device_ids(ids)
        if out is None:
            out = torch.empty(ids.numel(), self.n_cols, dtype=torch.float32, device=self.device)
        elif (out.dtype != torch.float32 or out.device != ids.device or out.shape != (ids.numel(), self.n_cols)
              or (out.numel() and (out.stride(1) != 1 and self.n_cols > 1 or out.stride(0) < self.n_cols))):
            raise ValueError("pyhgt_amd: out must be a float32 [n, %d] tensor on the graph's device with unit column stride" % self.n_cols)
        self._launch(ids, t_min, t_max, dist=out)
        return out

    def index(self, ids, t_min=None, t_max=None):
        """int64 [n]: the class of the first qualifying neighbour (the paper-venue script), -1 without one"""
        if self.device is None:
            return torch.from_numpy(np_label_index(self.g, self.triple, self.col_of, ids, t_min, t_max))
        ids = self._device_ids(ids)
        out = torch.empty(ids.numel(), dtype=torch.int32, device=self.device)
        self._launch(ids, t_min, t_max, index=out)
        return out.long()

    def columns(self, ids, t_min=None, t_max=None, width=None):
        """(columns int32 [n, width], count int32 [n]): row r's classes as a list in ascending order, -1 behind them -- the labels of
        `distribution` without the dense [n, C] matrix, for class_loss(columns=, count=).  count is the true number of classes; a row
        with more than `width` holds the first `width`.  width=None takes the largest count (at least 1), which costs one more launch
        and one host read; a given width makes no synchronisation."""
        if width is not None and int(width) < 1:
            raise ValueError("pyhgt_amd: width >= 1")
        if self.device is None:
            columns, count = np_label_columns(self.g, self.triple, self.col_of, ids, t_min, t_max, width)
            return torch.from_numpy(columns), torch.from_numpy(count)
        ids = self._device_ids(ids)
        count = torch.empty(ids.numel(), dtype=torch.int32, device=self.device)
        if width is None:
            self._launch(ids, t_min, t_max, count=count)
            width = max(int(count.max()) if ids.numel() else 0, 1)
        columns = torch.empty(ids.numel(), int(width), dtype=torch.int32, device=self.device)
        has, lo, hi = _window(t_min, t_max)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().hgt_sampler_label_columns(C.byref(self._triple_c), self.n_tgt, self.n_src,
                                                             ids.data_ptr() if ids.numel() else None, ids.numel(),
                                                             self.col_of_dev.data_ptr() if self.n_src else None, self.n_cols, has, lo, hi,
                                                             columns.data_ptr() if ids.numel() else None, int(width),
                                                             count.data_ptr() if ids.numel() else None,
                                                             torch.cuda.current_stream(self.device).cuda_stream), "hgt_sampler_label_columns")
            ids.record_stream(torch.cuda.current_stream(self.device))
        return columns, count

    def counts(self, ids, t_min=None, t_max=None):
        """int64 [n]: the number of distinct classes per row"""
        if self.device is None:
            return torch.from_numpy(np_label_counts(self.g, self.triple, self.col_of, ids, t_min, t_max))
        ids = self._device_ids(ids)
        out = torch.empty(ids.numel(), dtype=torch.int32, device=self.device)
        self._launch(ids, t_min, t_max, count=out)
        return out.long()

    def targets(self, t_min=None, t_max=None):
        """host numpy, for set-up time: (ids, times) of the target nodes with at least one qualifying neighbour, the time that of the
        first qualifying edge -- what train_pairs / valid_pairs / test_pairs of the scripts hold for a time range"""
        row, _, tm = _np_qualifying(self.g.csr[self.m], self.col_of, np.arange(self.n_tgt), t_min, t_max)
        ids, first = np.unique(row, return_index=True)
        return ids.astype(np.int64), tm[first].astype(np.int64)
