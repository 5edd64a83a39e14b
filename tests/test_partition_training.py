"""CPU tests of training on a destination partition (pyhgt_amd/dist.py): the index of the gradient return path
(HaloPlan.return_index), the reverse all-to-all with a torch reduce over gloo (HaloPlan.return_grads, HaloExchangeFunction), and
the C ABI of the kernel that adds the returned rows on the GPU (hgt_scatter_add_rows)."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pyhgt_amd import _lib
from pyhgt_amd.synth import synthetic_typed_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# -- return_index ------------------------------------------------------------------------------------------------------------
def _plan_with_send_rows(send_rows):
    from pyhgt_amd.dist import HaloPlan
    hp = HaloPlan.__new__(HaloPlan)
    hp.send_rows = torch.tensor(send_rows, dtype=torch.int32)
    return hp


def _return_index_numpy(send_rows):
    """The definition: the distinct rows ascending; per row its positions in the send list, ascending."""
    sr = np.asarray(send_rows, dtype=np.int64)
    rows = sorted(set(sr.tolist()))
    ptr, pos = [0], []
    for r in rows:
        pos.extend(np.nonzero(sr == r)[0].tolist())
        ptr.append(len(pos))
    return np.asarray(rows, np.int32), np.asarray(ptr, np.int32), np.asarray(pos, np.int32)


# world = 4, two chunks; the send list is in (chunk, peer, id) order.  Row 5: asked for by all world - 1 = 3 peers, by peer 1 in chunk 0
# and by peers 2 and 3 in chunk 1 (different chunks for different peers); row 2: by one peer; rows 0, 1, 3, 4, 6: by nobody; row 9:
# by two peers of the same chunk
HAND_MADE = [
    [2, 5, 9, 9, 5, 7, 5],            # chunk 0: peer 1 -> {2, 5}, peer 2 -> {9}, peer 3 -> {9}; chunk 1: peer 2 -> {5, 7}, peer 3 -> {5}
    [],                               # a rank nobody asks anything of
    [4],
    [3, 3, 3],                        # one row, every peer, one chunk
    list(range(20, 0, -1)) + list(range(1, 21)),      # descending then ascending: positions must still ascend within a row
]


@pytest.mark.parametrize("send_rows", HAND_MADE, ids=["chunks_and_peers", "empty", "single", "all_peers_one_row", "descending"])
def test_return_index_on_hand_made_send_lists(send_rows):
    rows, ptr, pos = _plan_with_send_rows(send_rows).return_index()
    assert rows.dtype == ptr.dtype == pos.dtype == torch.int32
    r_ref, p_ref, q_ref = _return_index_numpy(send_rows)
    assert np.array_equal(rows.numpy(), r_ref) and np.array_equal(ptr.numpy(), p_ref) and np.array_equal(pos.numpy(), q_ref)
    assert ptr.numel() == rows.numel() + 1 and int(ptr[0]) == 0 and int(ptr[-1]) == len(send_rows) == pos.numel()
    assert bool((rows[1:] > rows[:-1]).all())                      # strictly ascending: distinct rows
    for i in range(rows.numel()):
        seg = pos[int(ptr[i]):int(ptr[i + 1])]
        assert seg.numel() >= 1 and bool((seg[1:] > seg[:-1]).all())
        assert all(send_rows[p] == int(rows[i]) for p in seg.tolist())
    if send_rows == HAND_MADE[0]:
        mult = dict(zip(rows.tolist(), (ptr[1:] - ptr[:-1]).tolist()))
        assert mult == {2: 1, 5: 3, 7: 1, 9: 2} and 0 not in mult
        assert pos[int(ptr[1]):int(ptr[2])].tolist() == [1, 4, 6]      # row 5: chunk 0 / peer 1, chunk 1 / peer 2, chunk 1 / peer 3
    # built once
    hp = _plan_with_send_rows(send_rows)
    assert hp.return_index()[0] is hp.return_index()[0]


# -- the reverse all-to-all over gloo ------------------------------------------------------------------------------------------
def _grad_value(p, gid, d):
    """d_local of rank p at (global row gid, column c): small integers, so that every order of addition gives the same float."""
    c = torch.arange(d, dtype=torch.float32)
    return (p + 1.0) + 4.0 * (gid.to(torch.float32) % 5.0)[:, None] + 32.0 * (c % 3.0)[None, :]


def _torch_reduce(recv, rows, ptr, pos, d_own):
    """hgt_scatter_add_rows in torch: the rows of a destination row one after the other, in list order."""
    for i in range(rows.numel()):
        for p in pos[int(ptr[i]):int(ptr[i + 1])].tolist():
            d_own[int(rows[i])] += recv[p]


def _holders(ei, offsets, world):
    """holds[q] = the global ids rank q keeps as halo rows: remote sources of the in-edges of its targets."""
    out = []
    for q in range(world):
        lo, hi = offsets[q], offsets[q + 1]
        src = ei[0][(ei[1] >= lo) & (ei[1] < hi)]
        out.append(torch.unique(src[(src < lo) | (src >= hi)]))
    return out


def _return_worker(rank, world, port, N, E, d, offsets, n_chunks, first_use, tmpdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pyhgt_amd.dist import HaloPlan, HaloExchangeFunction, target_blocks
        torch.set_num_threads(2)
        x, nt, ei, et, tm = synthetic_typed_graph(N, E, d, 3, 4, seed=77, sorted_types=False)
        lo, hi = offsets[rank], offsets[rank + 1]
        mine = (ei[1] >= lo) & (ei[1] < hi)
        src_g, dst_l = ei[0][mine], ei[1][mine] - lo
        eblock = None
        if first_use:      # chunks by the first target block that uses a row (the blocked schedule's halo order)
            bounds = target_blocks(dst_l, hi - lo, n_chunks, align=16)
            eblock = torch.searchsorted(torch.tensor(bounds[1:]), dst_l, right=True).clamp(max=n_chunks - 1)
        hp = HaloPlan(nt[lo:hi], src_g, offsets, rank, world, n_chunks=n_chunks, edge_block=eblock)
        assert hp.n_own == hi - lo
        gid_local = torch.cat([torch.arange(lo, hi), hp.need[hp.halo_order]])          # global id of every local row
        d_local = _grad_value(rank, gid_local, d)
        # expected: my own contribution + that of every peer that holds the row
        expect = _grad_value(rank, torch.arange(lo, hi), d)
        n_contrib = torch.zeros(hi - lo, dtype=torch.int64)
        for q, held in enumerate(_holders(ei, offsets, world)):
            if q == rank:
                continue
            h = held[(held >= lo) & (held < hi)]
            expect[h - lo] += _grad_value(q, h, d)
            n_contrib[h - lo] += 1
        # (1) return_grads with a torch reduce; a rank with an empty range enters every collective like the others
        d_own = d_local[:hp.n_own].clone()
        with pytest.raises(RuntimeError, match="reduce"):
            hp.return_grads(d_local, d_own.clone())                 # CPU tensors without reduce= raise, before any collective
        out = hp.return_grads(d_local, d_own, reduce=_torch_reduce)
        assert out is d_own
        assert torch.equal(d_own, expect), "rank %d: %d rows differ" % (rank, int((d_own != expect).any(1).sum()))
        rows, ptr, pos = hp.return_index()
        assert torch.equal((ptr[1:] - ptr[:-1]).long(), n_contrib[rows.long()]) and int((n_contrib > 0).sum()) == rows.numel()
        # a second step reuses the persistent receive buffer
        d_own2 = d_local[:hp.n_own].clone()
        hp.return_grads(d_local, d_own2, reduce=_torch_reduce)
        assert torch.equal(d_own2, expect)
        # (2) the exchange as an autograd Function: d<x_local, w>/dx_own with w = d_local is the same sum
        x_own = x[lo:hi].clone().requires_grad_(True)
        x_local = HaloExchangeFunction.apply(hp, x_own, lambda xo, r: xo.index_select(0, r.long()), _torch_reduce)
        assert x_local.shape == (hp.n_local, d) and torch.equal(x_local.detach(), x[gid_local])
        (x_local * d_local).sum().backward()
        assert torch.equal(x_own.grad, expect)
        torch.save(torch.tensor([hp.n_own, hp.n_halo, int(n_contrib.max()) if hp.n_own else 0]), os.path.join(tmpdir, "ok%d.pt" % rank))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("first_use", [False, True], ids=["equal_slices", "first_use"])
@pytest.mark.parametrize("world,offsets", [(2, [0, 400, 900]), (3, [0, 250, 610, 900]), (4, [0, 300, 300, 620, 900])])
def test_halo_gradients_return_to_their_owners(world, offsets, first_use, tmp_path):
    """900 nodes / 9 000 edges over 2, 3 and 4 ranks (rank 1 of 4 owns nothing): every rank's d_own equals, exactly, its own
    gradient plus the closed-form sum over the peers that hold the row."""
    N, E, d, n_chunks = 900, 9000, 8, 3
    mp.spawn(_return_worker, args=(world, _free_port(), N, E, d, offsets, n_chunks, first_use, str(tmp_path)), nprocs=world, join=True)
    stats = [torch.load(os.path.join(str(tmp_path), "ok%d.pt" % r)) for r in range(world)]
    assert [int(s[0]) for s in stats] == [offsets[r + 1] - offsets[r] for r in range(world)]
    assert all(int(s[1]) > 0 for s in stats if int(s[0]) > 0)
    # some row is held by every peer that has targets: the return path really adds several contributions into one row
    assert max(int(s[2]) for s in stats) == sum(1 for r in range(world) if offsets[r + 1] > offsets[r]) - 1


# -- ABI -----------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_hgt_scatter_add_rows():
    text = open(os.path.join(ROOT, "include", "hgt_hip.h")).read()
    assert re.search(r"#define\s+HGT_ABI_VERSION\s+8\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+hgt_scatter_add_rows\s*\(([^)]*)\)\s*;", code)
    assert m, "include/hgt_hip.h does not declare hgt_scatter_add_rows"
    params = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert params == ["const float* src", "int64_t ld_src", "const int32_t* rows", "const int32_t* ptr", "const int32_t* pos",
                      "int64_t n_rows", "int32_t d", "float* dst", "int64_t ld_dst", "void* stream"]
    import ctypes as C
    ctype_of = lambda p: C.c_void_p if "*" in p else {"int64_t": C.c_int64, "int32_t": C.c_int32}[p.split()[0]]
    res, args = _lib.SIGNATURES["hgt_scatter_add_rows"]
    assert res is C.c_int and args == [ctype_of(p) for p in params]
    lib = _lib.load()
    assert hasattr(lib, "hgt_scatter_add_rows")
    assert _lib.ABI_VERSION == 8 and lib.hgt_abi_version() == 8
