// Index maps of the K-side logits kernel (hgt_edge_logits_kside.hip), shared by its pack kernel, the edge kernel and the host
// enumeration hgt_kside_image_map (tests/test_kside_image.py runs the maps on the CPU).
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
