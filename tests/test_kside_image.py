"""Host side of the K-side logits kernel (csrc/hgt_edge_logits_kside.hip): the index maps of its packed relation image and of
its lanes, enumerated by hgt_kside_image_map with the kernel's own helpers (csrc/hgt_kside_map.h), and the argument checks of
its entry points.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from pyhgt_amd import _lib

INVALID, UNSUPPORTED = -1, -2
BLOCK = 2 * 2 * 64 * 8          # f16 elements of one (relation, head) block


def _maps(n_blocks):
    lib = _lib.load()
    image = np.full((max(n_blocks, 1) * BLOCK, 4), -1, dtype=np.int32)
    b_col = np.full((2, 64, 8), -1, dtype=np.int32)
    c_out = np.full((64, 16), -1, dtype=np.int32)
    assert lib.hgt_kside_image_map(n_blocks, image.ctypes.data, b_col.ctypes.data, c_out.ctypes.data) == 0
    return image[:n_blocks * BLOCK], b_col, c_out


@pytest.mark.parametrize("R,H", [(1, 2), (3, 4), (8, 8)])
def test_image_is_a_bijection_of_the_relation_entries(R, H):
    """Every (relation, head, output, k) entry of att_t appears exactly once in the hi plane and once in the lo plane."""
    image, _, _ = _maps(R * H)
    assert image.min() >= 0
    blk, term, out, k = image.T
    assert blk.max() == R * H - 1 and set(term.tolist()) == {0, 1} and out.max() == 31 and k.max() == 31
    for t in (0, 1):
        sel = term == t
        key = (blk[sel].astype(np.int64) * 32 + out[sel]) * 32 + k[sel]
        assert key.size == R * H * 1024
        assert np.array_equal(np.sort(key), np.arange(R * H * 1024))
    # hi and lo of an entry sit at the same (k-step, lane, element) of their planes: one 16-byte load per lane and plane
    p = np.arange(image.shape[0])
    plane = (p // 512) % 2
    assert np.array_equal(plane, term)
    hi, lo = image[term == 0], image[term == 1]
    assert np.array_equal(hi[:, [0, 2, 3]], lo[:, [0, 2, 3]])


def test_a_lane_touches_16_consecutive_columns():
    """The 16 k values a lane supplies over the two k-steps and the 16 outputs it receives are columns 16 half .. + 15 of the head."""
    _, b_col, c_out = _maps(0)
    for lane in range(64):
        half = lane >> 5
        want = np.arange(16 * half, 16 * half + 16)
        assert np.array_equal(np.concatenate([b_col[0, lane], b_col[1, lane]]), want)
        assert np.array_equal(c_out[lane], want)


def test_mfma_lane_maps_over_the_packed_image_reproduce_the_transform():
    """numpy emulation of v_mfma_f32_32x32x16 (A: lane (i, half) holds A[i][8 half + j]; B: lane (n, half) holds B[8 half + j][n];
    C: lane (n, half), register reg holds C[(reg & 3) + 8 (reg >> 2) + 4 half][n]) over the packed image and a random K batch:
    every lane's register reg must hold output c_out[lane][reg] of  att_t[block] @ k  for the lane's edge."""
    rng = np.random.default_rng(5)
    n_blocks = 3
    image, b_col, c_out = _maps(n_blocks)
    att_t = rng.standard_normal((n_blocks, 32, 32))            # [block][output][k]
    packed = att_t[image[:, 0], image[:, 2], image[:, 3]].reshape(n_blocks, 2, 2, 64, 8)      # [block][k-step][term][lane][j]
    assert np.array_equal(packed[:, :, 0], packed[:, :, 1])    # (no split here: both planes carry the value)
    kbatch = rng.standard_normal((32, 32))                     # [edge][column of the head]
    lanes = np.arange(64)
    for blk in range(n_blocks):
        want = kbatch @ att_t[blk].T                           # [edge][output]
        Cm = np.zeros((32, 32))                                # logical [row][edge]
        for s in range(2):
            A = np.zeros((32, 16))
            B = np.zeros((16, 32))
            for j in range(8):
                A[lanes & 31, 8 * (lanes >> 5) + j] = packed[blk, s, 0, lanes, j]
                B[8 * (lanes >> 5) + j, lanes & 31] = kbatch[lanes & 31, b_col[s, lanes, j]]
            Cm += A @ B
        for reg in range(16):
            got = Cm[(reg & 3) + 8 * (reg >> 2) + 4 * (lanes >> 5), lanes & 31]
            assert np.allclose(got, want[lanes & 31, c_out[lanes, reg]], rtol=0, atol=1e-12)


def test_image_bytes():
    lib = _lib.load()
    nb = C.c_uint64(7)
    for R, H in [(8, 8), (3, 4), (2, 2)]:
        assert lib.hgt_relation_kside_bytes(R, H, 32, C.byref(nb)) == 0
        assert nb.value == R * H * BLOCK * 2 + (R * H * 4 + 255) // 256 * 256
    for R, H, dkp in [(4, 8, 64), (4, 16, 32), (4, 1, 64), (4, 4, 16)]:      # layouts the kernel does not cover: no image
        assert lib.hgt_relation_kside_bytes(R, H, dkp, C.byref(nb)) == 0 and nb.value == 0
    assert lib.hgt_relation_kside_bytes(0, 8, 32, C.byref(nb)) == INVALID
    assert lib.hgt_relation_kside_bytes(4, 8, 32, None) == INVALID


def test_argument_errors_return_codes():
    """Faulty arguments of the new entry points are answered with codes before anything touches the GPU."""
    lib = _lib.load()
    p = 4096          # a non-null address nobody dereferences: every call below fails its checks first
    ok = dict(plan=p, N=100, E=10, T=2, R=3, H=8, dkp=32, Q=p, K=p, rte=None, att_t=p, img=p, f16=1, logits=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.hgt_edge_logits_kside(a["plan"], a["N"], a["E"], a["T"], a["R"], a["H"], a["dkp"], a["Q"], a["K"], a["rte"], a["att_t"],
                                         a["img"], a["f16"], a["logits"], None)

    for bad in (dict(plan=None), dict(Q=None), dict(K=None), dict(img=None), dict(logits=None), dict(H=0), dict(H=3), dict(dkp=0),
                dict(R=0), dict(N=-1), dict(E=-1), dict(H=8, dkp=4)):
        assert call(**bad) == INVALID, bad
    for unsup in (dict(rte=p), dict(dkp=64), dict(H=16), dict(H=1, dkp=64), dict(N=(1 << 32) // (8 * 32 * 4))):
        assert call(**unsup) == UNSUPPORTED, unsup
    assert call(E=0, logits=None) == 0          # an edgeless graph: nothing to do, the per-edge array may be NULL
    assert lib.hgt_relation_kside_pack(None, 3, 8, 32, p, None) == INVALID
    assert lib.hgt_relation_kside_pack(p, 3, 8, 32, None, None) == INVALID
    assert lib.hgt_relation_kside_pack(p, 0, 8, 32, p, None) == INVALID
    assert lib.hgt_relation_kside_pack(p, 3, 8, 64, p, None) == UNSUPPORTED
    assert lib.hgt_kside_image_map(-1, None, None, None) == INVALID
