"""The graph build on the GPU (csrc/hgt_graph_build.hip): `DeviceHeteroGraph.from_edge_lists(device=...)` against the numpy rule
`np_edge_lists_to_csr`, array for array (integers: no tolerance); the sampler, the label kernel and a masked batch on the built graph
against the same calls on `from_reference_graph`'s graph of the same data; `neighbour_mean` against `np_neighbour_mean` in float64
within the bound of a k-term fp32 sum, and its bits against a second call and against one-row calls.  test_graph_build.py checks the
numpy rule itself against the reference script's dicts."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import test_graph_build as GB
from pyhgt_amd import DeviceHeteroGraph, LabelSpace, _lib, neighbour_mean, np_neighbour_mean, sample_subgraph_device, seed_edge_mask
from test_hgt_gpu import DEV

pytestmark = pytest.mark.gpu

TYPES = GB.TYPES
CHUNK = _lib.GRAPH_MEAN_CHUNK


def assert_device_graph_equals(dev, host):
    """a graph built on the device against a host graph: schema, every CSR array (device copy and lazy download), degrees"""
    assert dev._csr is None, "nothing was downloaded by the build"
    for ip, src, tm in dev.csr_dev:
        assert ip.dtype == src.dtype == tm.dtype == torch.int32 and ip.device == src.device == tm.device == torch.device(DEV)
        assert ip.is_contiguous() and src.is_contiguous() and tm.is_contiguous()
    GB.assert_same_graph(dev, host)                                       # reads dev.csr: the one download
    assert dev._csr is not None and dev.csr is dev.csr
    for c_dev, c_host in zip(dev.csr_dev, dev.csr):
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(c_dev, c_host))
    for t in dev.types:
        assert dev.degree[t].dtype == torch.int32 and np.array_equal(dev.degree[t].cpu().numpy(), host.degree[t]), t


def strided(a):
    """[2, E] as the (1, 2)-strided .t() view of an [E, 2] tensor"""
    return a.t().contiguous().t()


@pytest.mark.parametrize("E", [0, 1, 63, 64, 65, 257, 5000])
def test_device_build_equals_the_numpy_rule(E):
    sizes = {0: (3, 3, 3, 3, 3), 1: (3, 4, 3, 3, 3), 63: (40, 31, 7, 3, 5), 64: (17, 300, 5, 4, 3), 65: (300, 9, 64, 3, 3),
             257: (65, 64, 63, 3, 3), 5000: (300, 257, 129, 8, 3)}[E]
    n_nodes = dict(zip(TYPES, sizes))
    for dtype in (np.int64, np.int32):
        _, edges = GB.raw_relations(E, seed=E, n_nodes=n_nodes, dtype=dtype)
        et, nt = GB.times_for(edges, n_nodes, E)
        for case in ("paper_and_author_years", "edge_times", "edge_times_and_institution_years", "no_times"):
            etc, ntc = GB.TIME_CASES[case](et, nt)
            want = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, edges, etc, ntc)
            for where in ("host", "device"):
                for layout in (strided, torch.Tensor.contiguous):
                    put = (lambda a: a.to(DEV)) if where == "device" else (lambda a: a)
                    raw = OrderedDict((k, put(layout(torch.from_numpy(v)))) for k, v in edges.items())
                    if E > 1:
                        assert all(v.stride() == ((1, 2) if layout is strided else (E, 1)) for v in raw.values())
                    got = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, raw, etc and {k: put(torch.from_numpy(v)) for k, v in etc.items()},
                                                            ntc, device=DEV)
                    assert_device_graph_equals(got, want)
        got = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, edges, None, {"paper": nt["paper"]}, device=DEV, reverse=None)
        assert_device_graph_equals(got, DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, edges, None, {"paper": nt["paper"]}, reverse=None))


def _pairs_graph(ei, tm, n, device):
    key = ("paper", "cites", "paper")
    return DeviceHeteroGraph.from_edge_lists(["paper"], {"paper": n}, {key: ei}, {key: tm}, device=device)


@pytest.mark.parametrize("shape", ["adjacent", "far_apart", "row_of_one_pair", "one_row"])
def test_duplicate_shapes(shape):
    E, n = 9000, 300
    rng = np.random.default_rng(21)
    ei = np.stack([rng.integers(0, n, E), rng.integers(1, n, E)])
    tm = rng.integers(-50, 50, E).astype(np.int32)
    if shape == "adjacent":
        ei[:, 1::2] = ei[:, 0::2]                                         # every entry twice in a row, the copies' times differ
    elif shape == "far_apart":
        ei[:, 4500:] = ei[:, :4500]                                       # every copy 4 500 entries behind its original ...
        ei[:, [0, E - 1]] = np.array([[5, 5], [2, 2]])                    # ... and one pair at both ends of the input
    elif shape == "row_of_one_pair":
        ei[:, 1000:7000] = np.array([[7], [0]])                           # target 0 is never drawn above: 6 000 copies of (0, 7)
    else:
        ei[1] = 11                                                        # all E entries on one row, each source ~30 times
    got = _pairs_graph(torch.from_numpy(ei).to(DEV), torch.from_numpy(tm).to(DEV), n, DEV)
    want = _pairs_graph(ei, tm, n, None)
    assert_device_graph_equals(got, want)
    ip, src, t = want.csr[0]
    if shape == "adjacent":
        assert src.size <= E // 2
    elif shape == "far_apart":
        assert src[ip[2]] == 5 and t[ip[2]] == tm[E - 1]
    elif shape == "row_of_one_pair":
        assert ip[1] == 1 and src[0] == 7 and t[0] == tm[6999]
    else:
        assert ip[11] == 0 and ip[12] == src.size == n and np.all(ip[12:] == n)


@pytest.fixture(scope="module")
def twins():
    """the same raw data through from_edge_lists on the device and through the script's dicts and from_reference_graph"""
    n_nodes = {"paper": 120, "author": 90, "field": 20, "institution": 6, "venue": 2}
    _, edges = GB.raw_relations(900, seed=1, n_nodes=n_nodes)
    _, nt = GB.times_for(edges, n_nodes, 1)
    feats = GB.features(n_nodes)
    built = DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, {k: torch.from_numpy(v).to(DEV) for k, v in edges.items()},
                                              node_time={"paper": torch.from_numpy(nt["paper"]).to(DEV)},
                                              features={t: torch.from_numpy(f).to(DEV) for t, f in feats.items()}, device=DEV)
    ref = DeviceHeteroGraph.from_reference_graph(GB.script_graph(TYPES, edges, None, {"paper": nt["paper"]}), feats, device=DEV)
    return built, ref


def _assert_same_batch(a, b, types):
    for u, v in zip(list(a[:5]) + list(a.sorted), list(b[:5]) + list(b.sorted)):
        assert u.dtype == v.dtype and torch.equal(u, v)
    assert a[5] == b[5] and a[6] == b[6]
    for t in types:
        assert torch.equal(a.indxs[t], b.indxs[t]) and torch.equal(a.times[t], b.times[t])


def test_the_sampler_cannot_tell_the_difference(twins):
    built, ref = twins
    inp = {"paper": [[i, 2015] for i in range(8)]}
    a, b = (sample_subgraph_device(g, 2015, 2, 4, inp, seed=12, plan=False) for g in (built, ref))
    _assert_same_batch(a, b, TYPES)
    assert a[0].shape[0] > 20 and a.sorted[0].numel() > a[0].shape[0]     # nodes were added, edges beyond the self loops exist


def test_the_built_graph_drives_labels_and_masked_batches(twins):
    built, ref = twins
    triple = ("paper", "field", "rev_has_topic")
    ids = torch.arange(40)
    la, lb = (LabelSpace(g, triple, np.arange(10)).index(ids, t_max=2012) for g in (built, ref))
    assert torch.equal(la, lb) and (la >= 0).any() and (la < 0).any()
    inp = {"paper": [[i, 2015] for i in range(8)]}
    batches = [sample_subgraph_device(g, 2015, 2, 4, inp, seed=5, plan=False, mask=seed_edge_mask(g, ["has_topic", "rev_has_topic"], "paper", 8))
               for g in (built, ref)]
    _assert_same_batch(batches[0], batches[1], TYPES)
    plain = sample_subgraph_device(built, 2015, 2, 4, inp, seed=5, plan=False)
    assert batches[0].sorted[0].numel() < plain.sorted[0].numel()


# ---------------------------------------------------------------------------------------------------------------- neighbour mean
ROW_LENGTHS = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1, 2, 0, 3 * CHUNK]
N_SRC = 3 * CHUNK + 40


def _mean_edges(seed=0):
    """target rows of the lengths above, spread over two relations between the same type pair that share pairs (they count twice);
    no pair repeats inside a relation, so the row lengths are exact"""
    rng = np.random.default_rng(seed)
    first, second = [], []
    for r, k in enumerate(ROW_LENGTHS):
        in_second = 0 if k < 2 else (k // 3 if r % 2 else 1)              # the row's sequence: k - in_second terms, then in_second
        a = rng.permutation(N_SRC)[:k - in_second]
        b = np.concatenate([a[:in_second // 2], rng.permutation(N_SRC)])   # half of them shared with the first relation
        b = b[np.sort(np.unique(b, return_index=True)[1])][:in_second]
        first += [(s, r) for s in a]
        second += [(s, r) for s in b]
    order = rng.permutation(len(first))
    return OrderedDict([(("src", "a", "tgt"), np.array(first, dtype=np.int64)[order].T.copy()),
                        (("src", "b", "tgt"), np.array(second, dtype=np.int64).T.copy())])


@pytest.fixture(scope="module")
def mean_world():
    edges = _mean_edges()
    n_nodes = {"tgt": len(ROW_LENGTHS), "src": N_SRC}
    g = DeviceHeteroGraph.from_edge_lists(["tgt", "src"], n_nodes, edges, device=DEV)
    lengths = sum(np.diff(g.csr[m][0]) for m, (tt, st, _) in enumerate(g.triples) if (tt, st) == ("tgt", "src"))
    assert lengths.tolist() == ROW_LENGTHS
    shared = set(map(tuple, edges[("src", "a", "tgt")].T.tolist())) & set(map(tuple, edges[("src", "b", "tgt")].T.tolist()))
    assert len(shared) > 10
    return g, edges, n_nodes


def _place(x, layout):
    t = torch.from_numpy(x)
    if layout == "contiguous":
        return t.to(DEV)
    if layout == "left_columns":                                          # node_feature[:, :-1] of the script
        wide = torch.full((x.shape[0], x.shape[1] + 1), float("nan"))
        wide[:, :-1] = t
        return wide.to(DEV)[:, :-1]
    wide = torch.full((x.shape[0], x.shape[1] + 4), float("nan"))       # columns 1 .. d of a wider tensor: rows off their alignment
    wide[:, 1:1 + x.shape[1]] = t
    return wide.to(DEV)[:, 1:1 + x.shape[1]]


def _assert_mean_within_bound(g, x, got, tt="tgt", st="src"):
    """element by element within (k + 2) 2^-24 max_j |x_j|: a k-term fp32 sum in any order, the division, the stored rounding"""
    want = np_neighbour_mean(g, tt, st, x)
    n_rows = want.shape[0]
    k, biggest = np.zeros(n_rows), np.zeros_like(want)
    for m, (a, b, _) in enumerate(g.triples):
        if (a, b) == (tt, st):
            ip, src, _ = g.csr[m]
            k += np.diff(ip)
            np.maximum.at(biggest, np.repeat(np.arange(n_rows), np.diff(ip)), np.abs(x[src].astype(np.float64)))
    bound = (k + 2)[:, None] * 2.0 ** -24 * biggest
    err = np.abs(got.double().cpu().numpy() - want)
    worst = np.max(err / np.maximum(bound, 1e-300) * (bound > 0))
    print("neighbour_mean d=%d: worst error / bound = %.3f" % (x.shape[1], worst))
    assert np.all(err <= bound), (err - bound).max()
    assert np.array_equal(got.cpu().numpy()[k == 0], np.zeros(((k == 0).sum(), x.shape[1]), np.float32))
    return want


@pytest.mark.parametrize("layout", ["contiguous", "left_columns", "inner_columns"])
@pytest.mark.parametrize("d", [1, 3, 128, 129, 400])
def test_neighbour_mean_within_the_fp32_sum_bound(mean_world, d, layout):
    g, _, _ = mean_world
    x = np.random.default_rng(d).uniform(-1e4, 1e4, (N_SRC, d)).astype(np.float32)
    xd = _place(x, layout)
    got = neighbour_mean(g, "tgt", "src", xd)
    assert got.shape == (len(ROW_LENGTHS), d) and got.dtype == torch.float32
    want = _assert_mean_within_bound(g, x, got)
    assert np.abs(want).max() > 100                                        # a wrong order of magnitude would show
    # fixed bits: the same call again, and into the columns of a wider output
    assert torch.equal(got.view(torch.int32), neighbour_mean(g, "tgt", "src", xd).view(torch.int32))
    wide = torch.full((len(ROW_LENGTHS), d + 3), -7.0, device=DEV)
    assert neighbour_mean(g, "tgt", "src", xd, out=wide[:, 2:2 + d]).data_ptr() == wide[:, 2:2 + d].data_ptr()
    assert torch.equal(wide[:, 2:2 + d].contiguous().view(torch.int32), got.view(torch.int32))
    assert (wide[:, :2] == -7.0).all() and (wide[:, 2 + d:] == -7.0).all()


@pytest.mark.parametrize("d", [3, 128, 400])
def test_a_row_has_the_bits_of_its_one_row_call(mean_world, d):
    """the bits of a row depend on its own sequence of terms alone: each row again as the only row of a graph of its own"""
    g, edges, n_nodes = mean_world
    x = torch.from_numpy(np.random.default_rng(d + 1).uniform(-1e4, 1e4, (N_SRC, d)).astype(np.float32)).to(DEV)
    whole = neighbour_mean(g, "tgt", "src", x)
    for r in (2, 4, 5, 7, 8, 11):
        alone = OrderedDict()
        for key, ei in edges.items():
            sel = ei[:, ei[1] == r].copy()
            sel[1] = 0
            alone[key] = sel
        g1 = DeviceHeteroGraph.from_edge_lists(["tgt", "src"], {"tgt": 1, "src": N_SRC}, alone, device=DEV)
        one = neighbour_mean(g1, "tgt", "src", x)
        assert torch.equal(one.view(torch.int32)[0], whole.view(torch.int32)[r]), r


def test_mean_over_the_computed_rows_of_another_mean(mean_world):
    """the institution step of the script: the mean over rows that are themselves means (a column slice of a wider feature matrix)"""
    g, _, _ = mean_world
    x = torch.from_numpy(np.random.default_rng(9).uniform(-1e4, 1e4, (N_SRC, 16)).astype(np.float32)).to(DEV)
    tgt = torch.full((len(ROW_LENGTHS), 17), float("nan"), device=DEV)
    neighbour_mean(g, "tgt", "src", x, out=tgt[:, :-1])
    back = neighbour_mean(g, "src", "tgt", tgt[:, :-1])
    _assert_mean_within_bound(g, tgt[:, :-1].cpu().numpy(), back, "src", "tgt")


def test_argument_errors(mean_world):
    g, _, _ = mean_world
    x = torch.zeros(N_SRC, 8, device=DEV)
    with pytest.raises(ValueError):
        neighbour_mean(g, "tgt", "src", x[:-1])
    with pytest.raises(ValueError):
        neighbour_mean(g, "tgt", "src", x.double())
    with pytest.raises(ValueError):
        neighbour_mean(g, "tgt", "src", x, out=torch.zeros(len(ROW_LENGTHS), 9, device=DEV))
    with pytest.raises(KeyError):
        neighbour_mean(g, "tgt", "tgt", x)
    host = DeviceHeteroGraph.from_edge_lists(["tgt", "src"], {"tgt": 2, "src": 2}, {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        neighbour_mean(host, "tgt", "src", x)


@pytest.mark.parametrize("bad_id,row", [("n", 1), (-1, 1), ("n", 0), (-1, 0)])
def test_an_id_out_of_range_raises_and_names_the_relation(bad_id, row):
    n_nodes, edges = GB.raw_relations(400, seed=6)
    key = ("author", "writes", "paper")
    edges[key][row, 333] = n_nodes[key[2 if row else 0]] if bad_id == "n" else -1
    for dtype in (torch.int64, torch.int32):
        raw = OrderedDict((k, torch.from_numpy(v).to(DEV, dtype)) for k, v in edges.items())
        with pytest.raises(IndexError, match="writes"):
            DeviceHeteroGraph.from_edge_lists(TYPES, n_nodes, raw, device=DEV)
    torch.cuda.synchronize()
