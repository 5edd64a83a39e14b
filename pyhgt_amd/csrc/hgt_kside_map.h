// Index maps of the K-side logits kernel (hgt_edge_logits_kside.hip), shared by its pack kernel, the edge kernel and the host
// enumerations hgt_kside_image_map / hgt_kside_gather_map (tests/test_kside_image.py, tests/test_kside_gather_map.py run the maps on
// the CPU).
//
// Per (relation, head) the kernel evaluates  K~^T (32 outputs x 32 edges) = M (32 x 32) . K_h^T (32 x 32 edges)  with
// v_mfma_f32_32x32x16_f16, two k-steps.  M is the head's block of att_t -- M[out][k] = att_t[r][h][out][k], so that
// s_e,h = sum_out q[out] K~[out] -- with its rows and its k columns PERMUTED: both orders are free, and they are chosen so that a
// lane of the wavefront (edge = lane & 31, half = lane >> 5) touches 16 consecutive columns of the head's 128-byte line only:
//   B operand, k-step s, element j of lane (edge, half):   logical k = 16 s + 8 half + j   <-  column 16 half + 8 s + j of K[src]
//   C operand, register reg of lane (edge, half):          logical row (reg & 3) + 8 (reg >> 2) + 4 half  ->  output 16 half + reg
// i.e. the lane supplies columns 16 half .. + 15 of its edge's K row and receives outputs 16 half .. + 15, which it dots with
// the same 64 bytes of Q[dst].
//
// The lane's 64 bytes of K[src] and of Q[dst] reach it through LDS (the gather maps below): one LDS-DMA instruction -- a *piece* --
// fetches 8 edges x the head's whole 128-byte line, lanes 8 r .. 8 r + 7 the eight 16-byte chunks of edge 8 piece + r, and writes
// them to 16 lane of the piece's 1 KB.  Which chunk a lane fetches is chosen so that the four 16-byte reads of lane (edge, half) --
// chunks 4 half + i -- fall on 16 different 16-byte columns of the LDS in every lane group of a 128-bit read.
//
// Image: f16[R * H][k-step 2][term 2 = hi, lo][lane 64][8], the A operand of every (k-step, term) as one 16-byte load per lane,
// followed by int32[R * H]: the exponent that undoes the (relation, head) block's power-of-two scale.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HGT_KSIDE_HD __host__ __device__
#else
#define HGT_KSIDE_HD
#endif

constexpr int HGT_KSIDE_DK = 32;                       // the padded head width the kernel covers
constexpr int HGT_KSIDE_BLOCK_ELEMS = 2 * 2 * 64 * 8;  // f16 elements of one (relation, head) block: 4 KB

// logical row of the MFMA's A / C matrices -> output column of the head
HGT_KSIDE_HD constexpr int hgt_kside_row_out(int m) { return 16 * ((m >> 2) & 1) + (m & 3) + 4 * (m >> 3); }
// logical k of the MFMA (k-step s, lane half, element j) -> k column of the head
HGT_KSIDE_HD constexpr int hgt_kside_k_col(int s, int half, int j) { return 16 * half + 8 * s + j; }
// C operand: register reg of a lane of half `half` -> output column of the head
HGT_KSIDE_HD constexpr int hgt_kside_c_out(int half, int reg) { return hgt_kside_row_out((reg & 3) + 8 * (reg >> 2) + 4 * half); }

// element index of (block rh, k-step s, term, lane, j) in the image
HGT_KSIDE_HD constexpr int64_t hgt_kside_image_index(int64_t rh, int s, int term, int lane, int j) {
    return (((rh * 2 + s) * 2 + term) * 64 + lane) * 8 + j;
}
// ... and what the A operand holds there: lane (row m = lane & 31, half = lane >> 5) has M[m][16 s + 8 half + j]
HGT_KSIDE_HD constexpr int hgt_kside_image_out(int lane) { return hgt_kside_row_out(lane & 31); }
HGT_KSIDE_HD constexpr int hgt_kside_image_k(int s, int lane, int j) { return hgt_kside_k_col(s, lane >> 5, j); }

static_assert(hgt_kside_c_out(0, 0) == 0 && hgt_kside_c_out(0, 15) == 15 && hgt_kside_c_out(1, 0) == 16 && hgt_kside_c_out(1, 15) == 31,
              "a lane receives 16 consecutive outputs");

// Gather maps: a batch of 32 edges x one head line = 4 pieces of 1 KB, 64 slots of 16 bytes each.
// chunk c of row r (edge 8 p + r) of piece p lives in slot 8 r + (c ^ swizzle(p, r)) of the piece
HGT_KSIDE_HD constexpr int hgt_kside_gather_swizzle(int p, int r) { return 2 * (p & 3) + ((r >> 1) & 1); }
HGT_KSIDE_HD constexpr int hgt_kside_gather_slot(int p, int r, int c) { return 8 * r + (c ^ hgt_kside_gather_swizzle(p, r)); }
// DMA lane s of piece p (its 16 bytes land in slot s): the edge of the batch and the chunk of that edge's head line it fetches
HGT_KSIDE_HD constexpr int hgt_kside_dma_edge(int p, int s) { return 8 * p + (s >> 3); }
HGT_KSIDE_HD constexpr int hgt_kside_dma_chunk(int p, int s) { return (s & 7) ^ hgt_kside_gather_swizzle(p, s >> 3); }
// read i of lane (edge = lane & 31, half = lane >> 5): the chunk it must deliver and its byte offset in the batch's 4 KB
HGT_KSIDE_HD constexpr int hgt_kside_read_chunk(int lane, int i) { return 4 * (lane >> 5) + i; }
HGT_KSIDE_HD constexpr int hgt_kside_read_offset(int lane, int i) {
    return 1024 * ((lane & 31) >> 3) + 16 * hgt_kside_gather_slot((lane & 31) >> 3, lane & 7, hgt_kside_read_chunk(lane, i));
}
static_assert(hgt_kside_gather_slot(3, 7, hgt_kside_dma_chunk(3, 61)) == 61 && hgt_kside_dma_edge(3, 61) == 31,
              "a DMA lane fetches the chunk that belongs in its own slot");
