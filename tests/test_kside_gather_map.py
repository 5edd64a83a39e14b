"""Gather maps of the K-side logits kernel (csrc/hgt_kside_map.h), enumerated by hgt_kside_gather_map with the kernel's own
helpers: a batch of 32 edges x one 128-byte head line reaches the lanes through four LDS-DMA pieces of 1 KB (8 edges x a whole line
each) and four 16-byte LDS reads per lane.  No GPU."""
import numpy as np

from pyhgt_amd import _lib

# lane groups of one ds_read_b128 (one LDS cycle each when the 16 addresses fall on 16 different 16-byte columns of the 256-byte row)
_G0 = [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27]
_G1 = [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]
READ_GROUPS = [_G0, _G1, [l + 32 for l in _G0], [l + 32 for l in _G1]]


def _maps():
    lib = _lib.load()
    dma = np.full((4, 64, 2), -1, dtype=np.int32)
    read = np.full((4, 64, 3), -1, dtype=np.int32)
    assert lib.hgt_kside_gather_map(dma.ctypes.data, read.ctypes.data) == 0
    assert lib.hgt_kside_gather_map(None, None) == 0
    return dma, read


def _lds_image(dma):
    """(edge, chunk) found at every 16-byte slot of the batch's 4 KB: DMA lane s of piece p writes slot 64 p + s"""
    return dma.reshape(256, 2)


def test_the_pieces_fetch_every_chunk_of_every_edge_once():
    dma, _ = _maps()
    assert dma.min() >= 0 and dma[..., 0].max() == 31 and dma[..., 1].max() == 7
    key = dma[..., 0].astype(np.int64) * 8 + dma[..., 1]
    assert np.array_equal(np.sort(key.ravel()), np.arange(32 * 8))


def test_every_8_lane_group_of_a_piece_covers_one_whole_line_of_one_edge():
    dma, _ = _maps()
    for p in range(4):
        for g in range(8):
            edge, chunk = dma[p, 8 * g:8 * g + 8].T
            assert set(edge.tolist()) == {8 * p + g}
            assert sorted(chunk.tolist()) == list(range(8))


def test_a_read_returns_the_chunk_of_the_lanes_own_edge():
    dma, read = _maps()
    image = _lds_image(dma)
    for i in range(4):
        for lane in range(64):
            off, edge, chunk = read[i, lane]
            assert off % 16 == 0 and 0 <= off < 4096
            assert (edge, chunk) == (lane & 31, 4 * (lane >> 5) + i)
            assert tuple(image[off // 16]) == (edge, chunk)


def test_the_reads_are_free_of_bank_conflicts_in_every_lane_group():
    _, read = _maps()
    for i in range(4):
        for group in READ_GROUPS:
            cols = (read[i, group, 0] // 16) % 16
            assert len(set(cols.tolist())) == 16, (i, group, cols)


def test_the_lane_ends_up_with_the_columns_the_matrix_core_operand_wants():
    """Composed with b_col of hgt_kside_image_map: element j of k-step s of a lane is float 8 s + j of its four reads in order, and
    must be column b_col[s][lane][j] of the head line: columns 16 half .. + 15."""
    lib = _lib.load()
    dma, read = _maps()
    image = _lds_image(dma)
    b_col = np.full((2, 64, 8), -1, dtype=np.int32)
    assert lib.hgt_kside_image_map(0, None, b_col.ctypes.data, None) == 0
    for lane in range(64):
        cols = []
        for i in range(4):
            edge, chunk = image[read[i, lane, 0] // 16]
            assert edge == (lane & 31)
            cols += [4 * chunk + f for f in range(4)]          # a 16-byte chunk = four fp32 columns of the head
        half = lane >> 5
        assert cols == list(range(16 * half, 16 * half + 16))
        assert cols == b_col[0, lane].tolist() + b_col[1, lane].tolist()
