"""Seeded synthetic typed graphs in the wire format HGTConv.forward consumes.

The format is what the reference's sampler emits (/root/reference/pyHGT/data.py:212-256):
node_feature f32[N,d], node_type i64[N] (type-contiguous, ascending), edge_index
i64[2,E] delivered as the (1,2)-strided transpose of an [E,2] list (data.py:245,254),
edge_type i64[E], edge_time i64[E] in [0,240) (data.py:250).  The recipe follows
SURVEY.md section 8(d): uniform sources/targets (Poisson in-degree), relation
ids independent of node types (every (src_type, rel, dst_type) combination occurs).
"""
from collections import OrderedDict

import numpy as np
import torch


def synthetic_typed_graph(num_nodes, num_edges, dim, num_types, num_relations, seed=0,
                          sorted_types=True, strided_edge_index=True, dst_skew=0.0,
                          with_time=True, schema=False, device="cpu"):
    """Returns (node_feature, node_type, edge_index, edge_type, edge_time) on `device`.

    dst_skew > 0 draws targets from a Pareto-like law (hub nodes) instead of uniform;
    schema=True ties every relation to one fixed (src_type, dst_type) pair like real
    heterogeneous data (requires sorted_types).
    """
    g = torch.Generator().manual_seed(seed)
    N, E, T, R = num_nodes, num_edges, num_types, num_relations
    node_type = torch.randint(0, T, (N,), generator=g)
    if sorted_types:
        node_type = node_type.sort().values
    node_feature = torch.randn(N, dim, generator=g)
    edge_type = torch.randint(0, R, (E,), generator=g)
    if schema:
        if not sorted_types:
            raise ValueError("schema graphs need type-contiguous nodes")
        counts = torch.bincount(node_type, minlength=T)
        offs = torch.cumsum(counts, 0) - counts
        rel_src = torch.randint(0, T, (R,), generator=g)
        rel_dst = torch.randint(0, T, (R,), generator=g)
        u = torch.rand(E, generator=g)
        w = torch.rand(E, generator=g)
        st, dt = rel_src[edge_type], rel_dst[edge_type]
        src = offs[st] + (u * counts[st].clamp(min=1)).long().clamp(max=N - 1)
        dst = offs[dt] + (w * counts[dt].clamp(min=1)).long().clamp(max=N - 1)
    else:
        src = torch.randint(0, N, (E,), generator=g)
        if dst_skew > 0.0:
            u = torch.rand(E, generator=g).clamp_min(1e-9)
            dst = ((u ** (-1.0 / dst_skew) - 1.0) % N).long().clamp(0, N - 1)
            dst = torch.randperm(N, generator=g)[dst]
        else:
            dst = torch.randint(0, N, (E,), generator=g)
    if strided_edge_index:
        edge_index = torch.stack([src, dst], dim=1).contiguous().t()   # [2,E] view, strides (1,2)
    else:
        edge_index = torch.stack([src, dst], dim=0).contiguous()
    if with_time:
        edge_time = torch.randint(0, 240, (E,), generator=g)
    else:
        edge_time = torch.zeros(E, dtype=torch.long)
    out = (node_feature, node_type, edge_index, edge_type, edge_time)
    if device != "cpu":
        # .to() keeps the strides of edge_index
        out = tuple(t.to(device) for t in out)
    return out


def pick_check_targets(node_type, dst, n_random=1600, tile=64, seed=0):
    """Target rows for a sampled parity check of a LARGE graph: rows around every node-type boundary (mixed-type tiles of the
    fused update), the first and the last (ragged) tile, the rows of maximum / minimum in-degree, and `n_random` random rows.
    node_type / dst may live on any device; returns a sorted unique int64 tensor on that device."""
    N = int(node_type.numel())
    dev = node_type.device
    picks = [torch.arange(0, min(N, tile), device=dev), torch.arange(max(0, N - tile - 7), N, device=dev)]
    change = (node_type[1:] != node_type[:-1]).nonzero().flatten()[:16]          # type-sorted graphs: T-1 boundaries
    for b in change.tolist():
        picks.append(torch.arange(max(0, b - tile // 2), min(N, b + tile // 2), device=dev))
    deg = torch.bincount(dst, minlength=N)
    picks.append(deg.argmax().reshape(1))
    picks.append(deg.argmin().reshape(1))
    picks.append(torch.topk(deg, min(4, N)).indices)
    g = torch.Generator(device="cpu").manual_seed(seed)
    picks.append(torch.randint(0, N, (n_random,), generator=g).to(dev))
    return torch.unique(torch.cat([p.to(torch.int64) for p in picks]))


def induced_in_neighbourhood(node_feature, node_type, edge_index, edge_type, edge_time, targets):
    """The sub-graph that determines HGTConv's output rows `targets` exactly: ALL in-edges of those targets (original order)
    and the source nodes they reference, ids remapped to [0, n_sub).  A target's output depends on nothing else (softmax and
    aggregation are per target, conv.py:108-111; update is per node, conv.py:114-134), so an oracle run on this graph is
    exact for those rows -- the other nodes of the sub-graph lose in-edges and their outputs are meaningless.
    Returns CPU tensors (x_sub, node_type_sub, edge_index_sub [2,E_sub], edge_type_sub, edge_time_sub or None,
    pos) where pos[i] is the row of targets[i] in the sub-graph."""
    N = int(node_type.numel())
    dev = node_type.device
    src, dst = edge_index[0], edge_index[1]
    flag = torch.zeros(N, dtype=torch.bool, device=dev)
    flag[targets] = True
    eids = flag[dst].nonzero().flatten()
    s, t = src[eids], dst[eids]
    nodes = torch.unique(torch.cat([targets, s]))
    ei_sub = torch.stack([torch.searchsorted(nodes, s), torch.searchsorted(nodes, t)], dim=0)
    pos = torch.searchsorted(nodes, targets)
    tm = edge_time[eids].cpu() if edge_time is not None else None
    return (node_feature[nodes].cpu(), node_type[nodes].cpu(), ei_sub.cpu(), edge_type[eids].cpu(), tm, pos.cpu())


def synthetic_hetero_csr(types, meta, n_nodes, mean_degree=4.0, seed=0, years=(2000, 2020), none_time=()):
    """A random resident graph for the device sampler (pyhgt_amd.sampler.DeviceHeteroGraph.from_csr): per meta triple
    (target type, source type, relation) a CSR by target id -> (indptr, src, time) int32 arrays in `meta` order.

    A relation without the `rev_` prefix gets Poisson(mean_degree) distinct neighbours per target with one year per edge; its
    `rev_` twin (data.py:61) is the transpose with the same years, so a type with few nodes (venues, fields) has the long rows the
    reference's comment at data.py:106-111 speaks of.  Relations named in `none_time` carry no time (INT32_MIN, the reference's None)."""
    rng = np.random.default_rng(seed)
    meta = [tuple(m) for m in meta]
    coo = {}
    for tt, st, rel in meta:
        if rel.startswith("rev_"):
            continue
        n_t, n_s = int(n_nodes[tt]), int(n_nodes[st])
        if n_t == 0 or n_s == 0:
            coo[(tt, st, rel)] = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
            continue
        deg = np.minimum(rng.poisson(mean_degree, size=n_t), n_s)
        tgt = np.repeat(np.arange(n_t), deg)
        pair = np.unique(tgt * n_s + rng.integers(0, n_s, size=tgt.size))
        rng.shuffle(pair)                                                  # neighbours in no particular order, like a dict's
        tm = np.full(pair.size, -2 ** 31, np.int64) if rel in none_time else rng.integers(years[0], years[1], size=pair.size)
        coo[(tt, st, rel)] = (pair // n_s, pair % n_s, tm)
    out = []
    for tt, st, rel in meta:
        if rel.startswith("rev_") and (st, tt, rel[4:]) in coo:
            src, tgt, tm = coo[(st, tt, rel[4:])]
        else:
            tgt, src, tm = coo[(tt, st, rel)]
        order = np.argsort(tgt, kind="stable")
        indptr = np.concatenate([[0], np.cumsum(np.bincount(tgt, minlength=int(n_nodes[tt])))])
        out.append((indptr.astype(np.int32), src[order].astype(np.int32), tm[order].astype(np.int32)))
    return out


MAG_RAW_NODES = {"paper": 736389, "author": 1134649, "field_of_study": 59965, "institution": 8740}          # ogbn-mag
MAG_RAW_EDGES = OrderedDict([(("author", "affiliated_with", "institution"), 1043998), (("author", "writes", "paper"), 7145660),
                             (("paper", "cites", "paper"), 5416271), (("paper", "has_topic", "field_of_study"), 7505078)])


def synthetic_mag_raw(scale=1.0, feat_dim=128, seed=0):
    """ogbn-mag-shaped RAW arrays, the form OGB / PyG ship a heterogeneous dataset in: -> (types, n_nodes, edge_index_dict,
    paper features float32 [n_paper, feat_dim], paper years int32 [n_paper]) with node and edge counts `scale` times ogbn-mag's.
    edge_index_dict[(source type, relation, target type)] is an int64 [2, E] tensor in OGB's key order; the ends are drawn with a
    skew (squared uniforms), so that fields and institutions have the long rows of the real data, and pairs repeat now and then."""
    g = torch.Generator().manual_seed(seed)
    n_nodes = OrderedDict((t, max(4, int(n * scale))) for t, n in MAG_RAW_NODES.items())
    skewed = {"field_of_study", "institution"}
    edges = OrderedDict()
    for key, e in MAG_RAW_EDGES.items():
        E = max(1, int(e * scale))
        ends = []
        for t in (key[0], key[2]):
            u = torch.rand(E, generator=g, dtype=torch.float64)
            ends.append(((u * u if t in skewed else u) * n_nodes[t]).long().clamp_(max=n_nodes[t] - 1))
        edges[key] = torch.stack(ends)
    x = torch.randn(n_nodes["paper"], feat_dim, generator=g)
    years = torch.randint(2010, 2020, (n_nodes["paper"],), generator=g, dtype=torch.int32)
    return list(n_nodes), n_nodes, edges, x, years
