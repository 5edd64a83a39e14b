// Typed weight gradients of the backward pass (the derivation is in hgt_bwd_update.hip): dW[g] = A_g^T B_g as exact fp32 MFMA products
// (hgt_typed_wgrad) or 3-term split-bf16 ones (hgt_typed_wgrad_bf16x3, + the column sums), and the column sums alone
// (hgt_typed_colsum).  Each has one host function behind its atomic and its `_det` entry point (hgt_det.h).
#include "hgt_det.h"
#include "hgt_edge_common.h"
#include "hgt_split_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Typed weight gradient  dW[g][m][n] += sum_{rows p of group g} A[rows[p]][m] * B[rows[p]][n]   (= A_g^T B_g)
// on v_mfma_f32_32x32x2_f32 (exact fp32 products).  A workgroup owns a 64 x 64 tile of (m, n) and a chunk of WG_ROWS rows of
// one group: the 64-row slices of A and B go through LDS ([row][64] fp32), each wavefront owns a 32 x 32 quadrant, the
// partial tile is added to dW with fp32 atomics (one pass over every row per (m, n) tile: A is re-read n_out/64 times, B
// m/64 times -- fine for a one-off per step; the forward GEMMs are the optimised ones).
// ---------------------------------------------------------------------------------------------
constexpr int WG_ROWS = 2048;

// DET: chunk `slot % det_chunks` of the det_chunks equal row chunks (a multiple of `quantum` rows) of group `slot / det_chunks`
__device__ __forceinline__ void det_chunk_of(int slot, int det_chunks, int quantum, const int32_t* __restrict__ group_off, int& g,
                                             int& ch, int& p0, int& p1) {
    g = slot / det_chunks;
    ch = slot - g * det_chunks;
    const int gbeg = group_off[g], gend = group_off[g + 1];
    const int per = ((gend - gbeg + det_chunks - 1) / det_chunks + quantum - 1) / quantum * quantum;
    p0 = min(gbeg + ch * per, gend);
    p1 = min(p0 + per, gend);
}

#define HGT_WGRAD_KERNEL_PARAMS                                                                                                      \
    const float *__restrict__ A, int64_t lda, const float *__restrict__ B, int64_t ldb, const int32_t *__restrict__ rows,            \
        const int32_t *__restrict__ group_off, int n_groups, int M, int Nc, float *__restrict__ out, int64_t out_group_stride,       \
        int vecA, int vecB
#define HGT_WGRAD_KERNEL_ARGS A, lda, B, ldb, rows, group_off, n_groups, M, Nc, out, out_group_stride, vecA, vecB

template <bool DET>
__device__ __forceinline__ void typed_wgrad_body(HGT_WGRAD_KERNEL_PARAMS, int det_chunks) {
    __shared__ float sA[64][68];
    __shared__ float sB[64][68];
    // which (group, row chunk) is this block?
    int slot = blockIdx.x, g = 0, gbeg = 0, gend = 0, before = 0;
    int p0, p1, det_ch = 0;
    if constexpr (DET) {
        det_chunk_of(slot, det_chunks, 64, group_off, g, det_ch, p0, p1);
    } else {
        for (; g < n_groups; ++g) {
            gbeg = group_off[g];
            gend = group_off[g + 1];
            const int nch = (gend - gbeg + WG_ROWS - 1) / WG_ROWS;
            if (slot < before + nch) break;
            before += nch;
        }
        if (g >= n_groups) return;
        p0 = gbeg + (slot - before) * WG_ROWS;
        p1 = min(p0 + WG_ROWS, gend);
    }
    const int m0 = blockIdx.y * 64, n0 = blockIdx.z * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int pb = p0; pb < p1; pb += 64) {
        __syncthreads();
        // 64 rows x 64 columns of A and of B: thread -> (row = tid / 4 .. , 16 columns)
        {
            const int r = tid >> 2, cq = (tid & 3) * 16;
            const int p = pb + r;
            const int64_t rid = (p < p1) ? (int64_t)rows[p] : -1;
#pragma unroll
            for (int j = 0; j < 16; j += 4) {
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                if (rid >= 0) {
                    const int ma = m0 + cq + j, nb = n0 + cq + j;
                    if (vecA && ma + 3 < M) a = *reinterpret_cast<const float4*>(A + rid * lda + ma);
                    else { if (ma < M) a.x = A[rid * lda + ma]; if (ma + 1 < M) a.y = A[rid * lda + ma + 1]; if (ma + 2 < M) a.z = A[rid * lda + ma + 2]; if (ma + 3 < M) a.w = A[rid * lda + ma + 3]; }
                    if (vecB && nb + 3 < Nc) b = *reinterpret_cast<const float4*>(B + rid * ldb + nb);
                    else { if (nb < Nc) b.x = B[rid * ldb + nb]; if (nb + 1 < Nc) b.y = B[rid * ldb + nb + 1]; if (nb + 2 < Nc) b.z = B[rid * ldb + nb + 2]; if (nb + 3 < Nc) b.w = B[rid * ldb + nb + 3]; }
                }
                *reinterpret_cast<float4*>(&sA[r][cq + j]) = a;
                *reinterpret_cast<float4*>(&sB[r][cq + j]) = b;
            }
        }
        __syncthreads();
        // D[m][n] += sum_row A[row][m] B[row][n]: MFMA operand a = A^T[m = lane&31][k = row], b = B[k = row][n = lane&31]
#pragma unroll 8
        for (int k = 0; k < 64; k += 2) {
            const int kr = k + (lane >> 5);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[kr][wm + (lane & 31)], sB[kr][wn + (lane & 31)], acc, 0, 0, 0);
        }
    }
    // C layout: col (n) = lane & 31, row (m) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    // DET: this chunk's own [n_groups][M][Nc] slot (out = the workspace, out_group_stride = M * Nc; one chunk: out itself)
    float* o = out + (int64_t)g * out_group_stride + (DET ? (int64_t)det_ch * n_groups * out_group_stride : 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), n = n0 + wn + (lane & 31);
        if (m < M && n < Nc) {
            if constexpr (DET) o[(int64_t)m * Nc + n] = acc[r];
            else unsafeAtomicAdd(&o[(int64_t)m * Nc + n], acc[r]);
        }
    }
}

__global__ __launch_bounds__(256) void k_typed_wgrad(HGT_WGRAD_KERNEL_PARAMS) { typed_wgrad_body<false>(HGT_WGRAD_KERNEL_ARGS, 0); }
__global__ __launch_bounds__(256) void k_det_typed_wgrad(HGT_WGRAD_KERNEL_PARAMS, int det_chunks) {
    typed_wgrad_body<true>(HGT_WGRAD_KERNEL_ARGS, det_chunks);
}
#undef HGT_WGRAD_KERNEL_PARAMS
#undef HGT_WGRAD_KERNEL_ARGS

// ---------------------------------------------------------------------------------------------
// The same weight gradient as 3-term split-bf16 products on v_mfma_f32_32x32x16_bf16 (relative error of a product ~3 * 2^-18, like
// the forward typed linears): 8x the matrix-core rate of the fp32 instruction and 128 x 128 output tiles, so that A and B are
// re-read Nc/128 and M/128 times instead of Nc/64 and M/64 (the fp32 kernel above moved 33 GB per training step at c2 = 11 ms).
// Both MFMA operands need the ROW index along K, i.e. eight consecutive rows of one column per lane: the 32-row chunks of A and B
// are therefore staged through LDS TRANSPOSED -- a thread reads eight rows of one column (coalesced 256 B per wavefront and row),
// splits them into bf16 hi / mid and writes one 16 B fragment piece per plane; column stride 80 B: conflict-free writes and reads.
// The next chunk's rows are in flight (registers) while the current one is multiplied.  Optionally also the column sums of A
// (bias gradient), from the registers that pass through anyway.
// ---------------------------------------------------------------------------------------------
constexpr int WX_T = 128;            // tile edge (columns of A = rows of dW, columns of B)
constexpr int WX_KR = 32;            // rows per chunk
constexpr int WX_CS = 80;            // LDS bytes per column: 32 rows x 2 B + 16 B of padding
constexpr int WX_PLANE = WX_T * WX_CS;
constexpr int WX_ROWS = 4096;        // rows of one group per workgroup

#define HGT_WGRAD_X3_KERNEL_PARAMS                                                                                                   \
    const float *__restrict__ A, int64_t lda, const float *__restrict__ B, int64_t ldb, const int32_t *__restrict__ rows,            \
        const int32_t *__restrict__ group_off, int n_groups, int M, int Nc, int n_mt, float *__restrict__ out,                       \
        int64_t out_group_stride, float *__restrict__ colsum, int64_t cs_group_stride
#define HGT_WGRAD_X3_KERNEL_ARGS A, lda, B, ldb, rows, group_off, n_groups, M, Nc, n_mt, out, out_group_stride, colsum, cs_group_stride

template <bool DET>
__device__ __forceinline__ void typed_wgrad_x3_body(HGT_WGRAD_X3_KERNEL_PARAMS, int det_chunks) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * WX_PLANE];   // A hi | A mid | B hi | B mid
    // tile index fastest: the workgroups that share a row chunk are neighbours in launch order (their rows meet in the L2)
    const int mt = blockIdx.x % n_mt, nt = blockIdx.x / n_mt;
    int slot = blockIdx.y, g = 0, gbeg = 0, gend = 0, before = 0;
    int p0, p1, det_ch = 0;
    if constexpr (DET) {
        det_chunk_of(slot, det_chunks, WX_KR, group_off, g, det_ch, p0, p1);
    } else {
        for (; g < n_groups; ++g) {
            gbeg = group_off[g];
            gend = group_off[g + 1];
            const int nch = (gend - gbeg + WX_ROWS - 1) / WX_ROWS;
            if (slot < before + nch) break;
            before += nch;
        }
        if (g >= n_groups) return;
        p0 = gbeg + (slot - before) * WX_ROWS;
        p1 = min(p0 + WX_ROWS, gend);
    }
    const int m0 = mt * WX_T, n0 = nt * WX_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    // staging role: column c of the tile, row octets o0 and o0 + 2 of the chunk, for A and for B
    const int c = tid & 127, o0 = tid >> 7;
    const bool a_ok = m0 + c < M, b_ok = n0 + c < Nc;
    const float* __restrict__ pa = A + (a_ok ? m0 + c : 0);
    const float* __restrict__ pb = B + (b_ok ? n0 + c : 0);
    float va[16], vb[16];
    int rid[16], rid_next[16];       // row ids of the chunk in flight / of the one after it (no id -> row dependency inside the loop)
    auto load_ids = [&](int pbase, int (&ids)[16]) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int p = pbase + 8 * (o0 + 2 * (j >> 3)) + (j & 7);
            ids[j] = (p < p1) ? rows[p] : -1;
        }
    };
    auto load_rows = [&]() {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t r = max(rid[j], 0);
            va[j] = pa[r * lda];
            vb[j] = pb[r * ldb];
        }
    };
    float csum = 0.0f;
    auto commit = [&]() {       // registers -> transposed bf16 hi / mid planes (rows beyond the chunk and columns beyond M / Nc: 0)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float fa[8], fb[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool live = rid[half * 8 + j] >= 0;
                fa[j] = (live && a_ok) ? va[half * 8 + j] : 0.0f;
                fb[j] = (live && b_ok) ? vb[half * 8 + j] : 0.0f;
                csum += fa[j];
            }
            uint4 ah, am, bh, bm;
            split2(fa[0], fa[1], ah.x, am.x); split2(fa[2], fa[3], ah.y, am.y); split2(fa[4], fa[5], ah.z, am.z); split2(fa[6], fa[7], ah.w, am.w);
            split2(fb[0], fb[1], bh.x, bm.x); split2(fb[2], fb[3], bh.y, bm.y); split2(fb[4], fb[5], bh.z, bm.z); split2(fb[6], fb[7], bh.w, bm.w);
            unsigned char* w = smem + c * WX_CS + (o0 + 2 * half) * 16;
            *reinterpret_cast<uint4*>(w) = ah;
            *reinterpret_cast<uint4*>(w + WX_PLANE) = am;
            *reinterpret_cast<uint4*>(w + 2 * WX_PLANE) = bh;
            *reinterpret_cast<uint4*>(w + 3 * WX_PLANE) = bm;
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    load_ids(p0, rid);
    load_rows();
    load_ids(p0 + WX_KR, rid_next);
    for (int pbase = p0; pbase < p1; pbase += WX_KR) {
        __syncthreads();                 // the previous chunk's fragments have been read
        commit();
        if (pbase + WX_KR < p1) {        // next chunk's rows (in flight during the products below), the ids of the one after it
#pragma unroll
            for (int j = 0; j < 16; ++j) rid[j] = rid_next[j];
            load_rows();
            load_ids(pbase + 2 * WX_KR, rid_next);
        }
        __syncthreads();
        const unsigned char* fa = smem + (wm + (lane & 31)) * WX_CS + (lane >> 5) * 16;
        const unsigned char* fb = smem + 2 * WX_PLANE + (wn + (lane & 31)) * WX_CS + (lane >> 5) * 16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 ah[2], am[2], bh[2], bm[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *reinterpret_cast<const bf16x8*>(fa + i * 32 * WX_CS + ks * 32);
                am[i] = *reinterpret_cast<const bf16x8*>(fa + WX_PLANE + i * 32 * WX_CS + ks * 32);
                bh[i] = *reinterpret_cast<const bf16x8*>(fb + i * 32 * WX_CS + ks * 32);
                bm[i] = *reinterpret_cast<const bf16x8*>(fb + WX_PLANE + i * 32 * WX_CS + ks * 32);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
    }
    // C layout of a 32 x 32 tile: col (n) = lane & 31, row (m) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    // DET: this chunk's own [n_groups][M][Nc] / [n_groups][M] slots (out / colsum = the workspace; one chunk: the outputs themselves)
    float* o = out + (int64_t)g * out_group_stride + (DET ? (int64_t)det_ch * n_groups * out_group_stride : 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), n = n0 + wn + 32 * j + (lane & 31);
                if (m < M && n < Nc) {
                    if constexpr (DET) o[(int64_t)m * Nc + n] = acc[i][j][r];
                    else unsafeAtomicAdd(&o[(int64_t)m * Nc + n], acc[i][j][r]);
                }
            }
    if constexpr (DET) {
        // a column's sum sits in two threads (row octets o0 and o0 + 2 of every chunk): combined through LDS in a fixed order
        if (colsum && nt == 0) {      // (workgroup-uniform)
            float* s_cs = reinterpret_cast<float*>(smem);
            __syncthreads();          // the last chunk's fragments have been read
            if (o0 == 1) s_cs[c] = csum;
            __syncthreads();
            if (o0 == 0 && a_ok) colsum[((int64_t)det_ch * n_groups + g) * cs_group_stride + m0 + c] = csum + s_cs[c];
        }
    } else {
        if (colsum && nt == 0 && a_ok) unsafeAtomicAdd(&colsum[(int64_t)g * cs_group_stride + m0 + c], csum);
    }
}

__global__ __launch_bounds__(256) void k_typed_wgrad_x3(HGT_WGRAD_X3_KERNEL_PARAMS) { typed_wgrad_x3_body<false>(HGT_WGRAD_X3_KERNEL_ARGS, 0); }
__global__ __launch_bounds__(256) void k_det_typed_wgrad_x3(HGT_WGRAD_X3_KERNEL_PARAMS, int det_chunks) {
    typed_wgrad_x3_body<true>(HGT_WGRAD_X3_KERNEL_ARGS, det_chunks);
}
#undef HGT_WGRAD_X3_KERNEL_PARAMS
#undef HGT_WGRAD_X3_KERNEL_ARGS

// out[g][c] += sum_{rows p of group g} A[rows[p]][c]    (bias gradients)
__global__ __launch_bounds__(256) void k_typed_colsum(const float* __restrict__ A, int64_t lda, const int32_t* __restrict__ rows,
                                                      const int32_t* __restrict__ group_off, int n_groups, int M, float* __restrict__ out,
                                                      int64_t out_group_stride) {
    constexpr int CH = 256;
    int slot = blockIdx.x * 4 + (threadIdx.x >> 6), g = 0, gbeg = 0, gend = 0, before = 0;
    for (; g < n_groups; ++g) {
        gbeg = group_off[g];
        gend = group_off[g + 1];
        const int nch = (gend - gbeg + CH - 1) / CH;
        if (slot < before + nch) break;
        before += nch;
    }
    if (g >= n_groups) return;
    const int lane = threadIdx.x & 63;
    const int p0 = gbeg + (slot - before) * CH, p1 = min(p0 + CH, gend);
    for (int c0 = 0; c0 < M; c0 += 64 * 4) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int p = p0; p < p1; ++p) {
            const int64_t rid = rows[p];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j * 64 + lane;
                if (c < M) s[j] += A[rid * lda + c];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j * 64 + lane;
            if (c < M) unsafeAtomicAdd(&out[(int64_t)g * out_group_stride + c], s[j]);
        }
    }
}

// deterministic form: wavefront = chunk `slot % det_chunks` of group `slot / det_chunks`, its sums stored into the chunk's own
// [n_groups][out_group_stride] slot of `out` (the workspace; one chunk: the output itself)
__global__ __launch_bounds__(256) void k_det_typed_colsum(const float* __restrict__ A, int64_t lda, const int32_t* __restrict__ rows,
                                                          const int32_t* __restrict__ group_off, int n_groups, int M,
                                                          float* __restrict__ out, int64_t out_group_stride, int det_chunks) {
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= n_groups * det_chunks) return;
    int g, ch, p0, p1;
    det_chunk_of(slot, det_chunks, 1, group_off, g, ch, p0, p1);
    const int lane = threadIdx.x & 63;
    float* o = out + ((int64_t)ch * n_groups + g) * out_group_stride;
    for (int c0 = 0; c0 < M; c0 += 64 * 4) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int p = p0; p < p1; ++p) {
            const int64_t rid = rows[p];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j * 64 + lane;
                if (c < M) s[j] += A[rid * lda + c];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j * 64 + lane;
            if (c < M) o[c] = s[j];
        }
    }
}

constexpr int CS_ROWS = 256;         // rows per wavefront of k_typed_colsum (its CH)

// ---- host side: one function per step behind its atomic and its `_det` entry point
#define HGT_WGRAD_PARAMS                                                                                                       \
    const float *A, int64_t lda, const float *B, int64_t ldb, const int32_t *rows, const int32_t *group_off, int32_t n_groups, \
        int64_t n_rows, int32_t m, int32_t n_cols, float *out, int64_t out_group_stride
#define HGT_WGRAD_ARGS A, lda, B, ldb, rows, group_off, n_groups, n_rows, m, n_cols, out, out_group_stride
#define HGT_COLSUM_PARAMS                                                                                                      \
    const float *A, int64_t lda, const int32_t *rows, const int32_t *group_off, int32_t n_groups, int64_t n_rows, int32_t m,   \
        float *out, int64_t out_group_stride
#define HGT_COLSUM_ARGS A, lda, rows, group_off, n_groups, n_rows, m, out, out_group_stride

inline bool wgrad_sizes_bad(int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols) {
    return n_groups <= 0 || n_rows < 0 || m <= 0 || n_cols <= 0;
}

// Launch geometry.  The atomic forms launch an upper bound of fixed-size row chunks (the group sizes live on the device) ...
inline int64_t wgrad_chunk_bound(int n_groups, int64_t n_rows, int64_t chunk_rows) { return (n_rows + chunk_rows - 1) / chunk_rows + n_groups; }
// ... the det forms `chunks` equal row chunks per group, the slots of their workspace.  Weight gradient: budget = max(DET_FLOOR, 1/16
// of the bytes of A and B); a slot holds the weight partials and (bf16 x3 form: with_colsum) the column-sum partials; chunks x groups
// stays inside the grid's y / x extent
inline int64_t det_wgrad_chunks(int n_groups, int64_t n_rows, int m, int n_cols, int64_t chunk_rows, bool with_colsum) {
    const uint64_t budget = max(DET_FLOOR, (uint64_t)n_rows * (uint64_t)(m + n_cols) * 4 / 16);
    int64_t want = (n_rows + chunk_rows - 1) / chunk_rows;
    if (want > 1024) want = 1024;
    if (want > 65535 / n_groups) want = 65535 / n_groups;
    return det_fit_slots(want < 1 ? 1 : want, (uint64_t)n_groups * m * (n_cols + (with_colsum ? 1 : 0)), budget);
}
// column sums: chunks of >= 256 rows, at most 1024 per group, inside DET_FLOOR / 2
inline int64_t det_colsum_chunks(int n_groups, int64_t n_rows, int m) {
    int64_t want = (n_rows + CS_ROWS - 1) / CS_ROWS;
    if (want > 1024) want = 1024;
    return det_fit_slots(want < 1 ? 1 : want, (uint64_t)n_groups * m, DET_FLOOR / 2);
}
// one chunk per group needs no workspace: the kernel stores into the output itself
inline uint64_t det_chunk_ws_floats(int64_t chunks, uint64_t elems) { return chunks > 1 ? det_ws_floats(chunks, elems) : 0; }

// zero the [n_groups][per] blocks of a grouped output (group stride ogs floats)
void det_zero_groups(float* out, int n_groups, int64_t per, int64_t ogs, hipStream_t st) {
    (void)hipMemset2DAsync(out, (size_t)ogs * 4, 0, (size_t)per * 4, (size_t)n_groups, st);
}

// hgt_typed_wgrad_det_bytes (x3 = false) / hgt_typed_wgrad_bf16x3_det_bytes
int wgrad_det_bytes(bool x3, int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, uint64_t* out) {
    if (!out || wgrad_sizes_bad(n_groups, n_rows, m, n_cols)) return HGT_ERR_INVALID_ARG;
    if (n_groups > 65535) return HGT_ERR_TOO_LARGE;
    const int64_t chunks = det_wgrad_chunks(n_groups, n_rows, m, n_cols, x3 ? WX_ROWS : WG_ROWS, x3);
    // the weight partials, then (bf16 x3) the column-sum partials: always provided for, the size does not depend on the colsum argument
    *out = (det_chunk_ws_floats(chunks, (uint64_t)n_groups * m * n_cols) + (x3 ? det_chunk_ws_floats(chunks, (uint64_t)n_groups * m) : 0)) * 4;
    return HGT_OK;
}
}  // namespace

extern "C" int hgt_typed_colsum_det_bytes(int32_t n_groups, int64_t n_rows, int32_t m, uint64_t* out) {
    if (!out || wgrad_sizes_bad(n_groups, n_rows, m, 1)) return HGT_ERR_INVALID_ARG;
    *out = det_chunk_ws_floats(det_colsum_chunks(n_groups, n_rows, m), (uint64_t)n_groups * m) * 4;
    return HGT_OK;
}

// hgt_typed_wgrad[_det] (x3 = false: exact fp32 products, no colsum) and hgt_typed_wgrad_bf16x3[_det]; det == NULL: the atomic form
static int typed_wgrad_impl(bool x3, HGT_WGRAD_PARAMS, float* colsum, int64_t colsum_group_stride, const HgtDetWs* det, void* stream) {
    if (!A || !B || !rows || !group_off || !out || wgrad_sizes_bad(n_groups, n_rows, m, n_cols)) return HGT_ERR_INVALID_ARG;
    const int64_t per = (int64_t)m * n_cols, elems = per * n_groups, cs_elems = (int64_t)m * n_groups;
    if (det) {      // (only the det forms, which overwrite their outputs, have ever looked at the strides)
        if (out_group_stride < per || (colsum && colsum_group_stride < m)) return HGT_ERR_INVALID_ARG;
        uint64_t need = 0;
        if (int rc = wgrad_det_bytes(x3, n_groups, n_rows, m, n_cols, &need)) return rc;
        if (int rc = det_ws_check(*det, need)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        if (!det) return HGT_OK;
        det_zero_groups(out, n_groups, per, out_group_stride, st);
        if (colsum) det_zero_groups(colsum, n_groups, m, colsum_group_stride, st);
        HGT_CHECK_LAUNCH();
        return HGT_OK;
    }
    const int64_t chunk_rows = x3 ? WX_ROWS : WG_ROWS;
    const int64_t chunks = det ? det_wgrad_chunks(n_groups, n_rows, m, n_cols, chunk_rows, x3) : 0;
    const int64_t slots = det ? chunks * n_groups : wgrad_chunk_bound(n_groups, n_rows, chunk_rows);
    // det: the partials of `chunks` > 1 chunks go to the workspace ([chunk][group][m][n_cols], then the column sums' [chunk][group][m])
    float* part = chunks > 1 ? (float*)det->ptr : out;
    float* cs_part = chunks > 1 ? part + det_ws_floats(chunks, (uint64_t)elems) : colsum;
    const int64_t part_gs = chunks > 1 ? per : out_group_stride, cs_gs = chunks > 1 ? (int64_t)m : colsum_group_stride;
    if (x3) {
        const int n_mt = (m + WX_T - 1) / WX_T, n_nt = (n_cols + WX_T - 1) / WX_T;
        if (slots > 65535) return HGT_ERR_TOO_LARGE;      // (grid.y; the det chunk count is cut to fit)
        dim3 grid((unsigned)(n_mt * n_nt), (unsigned)slots);
        if (det)
            k_det_typed_wgrad_x3<<<grid, 256, 0, st>>>(A, lda, B, ldb, rows, group_off, n_groups, m, n_cols, n_mt, part, part_gs,
                                                      colsum ? cs_part : nullptr, cs_gs, (int)chunks);
        else
            k_typed_wgrad_x3<<<grid, 256, 0, st>>>(A, lda, B, ldb, rows, group_off, n_groups, m, n_cols, n_mt, out, out_group_stride, colsum,
                                                  colsum_group_stride);
    } else {
        const int vecA = ((lda & 3) == 0 && ((uintptr_t)A & 15) == 0), vecB = ((ldb & 3) == 0 && ((uintptr_t)B & 15) == 0);   // 16 B row loads
        dim3 grid((unsigned)slots, (unsigned)((m + 63) / 64), (unsigned)((n_cols + 63) / 64));
        if (det)
            k_det_typed_wgrad<<<grid, 256, 0, st>>>(A, lda, B, ldb, rows, group_off, n_groups, m, n_cols, part, part_gs, vecA, vecB, (int)chunks);
        else
            k_typed_wgrad<<<grid, 256, 0, st>>>(A, lda, B, ldb, rows, group_off, n_groups, m, n_cols, out, out_group_stride, vecA, vecB);
    }
    if (chunks > 1) {
        det_reduce(part, chunks, elems, elems, part + chunks * elems, out, per, out_group_stride, st);
        if (colsum) det_reduce(cs_part, chunks, cs_elems, cs_elems, cs_part + chunks * cs_elems, colsum, m, colsum_group_stride, st);
    }
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

// hgt_typed_colsum (det == NULL) and hgt_typed_colsum_det: a wavefront per row chunk
static int typed_colsum_impl(HGT_COLSUM_PARAMS, const HgtDetWs* det, void* stream) {
    if (!A || !rows || !group_off || !out || wgrad_sizes_bad(n_groups, n_rows, m, 1)) return HGT_ERR_INVALID_ARG;
    if (det) {      // (only the det form, which overwrites its output, has ever looked at the stride)
        if (out_group_stride < m) return HGT_ERR_INVALID_ARG;
        uint64_t need = 0;
        hgt_typed_colsum_det_bytes(n_groups, n_rows, m, &need);
        if (int rc = det_ws_check(*det, need)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        if (!det) return HGT_OK;
        det_zero_groups(out, n_groups, m, out_group_stride, st);
        HGT_CHECK_LAUNCH();
        return HGT_OK;
    }
    if (det) {
        const int64_t chunks = det_colsum_chunks(n_groups, n_rows, m), elems = (int64_t)m * n_groups;
        float* part = chunks > 1 ? (float*)det->ptr : out;
        k_det_typed_colsum<<<nblk(chunks * n_groups, 4), 256, 0, st>>>(A, lda, rows, group_off, n_groups, m, part,
                                                                       chunks > 1 ? (int64_t)m : out_group_stride, (int)chunks);
        if (chunks > 1) det_reduce(part, chunks, elems, elems, part + chunks * elems, out, m, out_group_stride, st);
    } else {
        k_typed_colsum<<<nblk(wgrad_chunk_bound(n_groups, n_rows, CS_ROWS), 4), 256, 0, st>>>(A, lda, rows, group_off, n_groups, m, out,
                                                                                            out_group_stride);
    }
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_typed_wgrad_det_bytes(int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, uint64_t* out) {
    return wgrad_det_bytes(false, n_groups, n_rows, m, n_cols, out);
}
extern "C" int hgt_typed_wgrad_bf16x3_det_bytes(int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, uint64_t* out) {
    return wgrad_det_bytes(true, n_groups, n_rows, m, n_cols, out);
}

extern "C" int hgt_typed_wgrad(HGT_WGRAD_PARAMS, void* stream) { return typed_wgrad_impl(false, HGT_WGRAD_ARGS, nullptr, 0, nullptr, stream); }
extern "C" int hgt_typed_wgrad_det(HGT_WGRAD_PARAMS, void* ws, uint64_t ws_bytes, void* stream) {
    const HgtDetWs det = {ws, ws_bytes};
    return typed_wgrad_impl(false, HGT_WGRAD_ARGS, nullptr, 0, &det, stream);
}
extern "C" int hgt_typed_wgrad_bf16x3(HGT_WGRAD_PARAMS, float* colsum, int64_t colsum_group_stride, void* stream) {
    return typed_wgrad_impl(true, HGT_WGRAD_ARGS, colsum, colsum_group_stride, nullptr, stream);
}
extern "C" int hgt_typed_wgrad_bf16x3_det(HGT_WGRAD_PARAMS, float* colsum, int64_t colsum_group_stride, void* ws, uint64_t ws_bytes,
                                          void* stream) {
    const HgtDetWs det = {ws, ws_bytes};
    return typed_wgrad_impl(true, HGT_WGRAD_ARGS, colsum, colsum_group_stride, &det, stream);
}
extern "C" int hgt_typed_colsum(HGT_COLSUM_PARAMS, void* stream) { return typed_colsum_impl(HGT_COLSUM_ARGS, nullptr, stream); }
extern "C" int hgt_typed_colsum_det(HGT_COLSUM_PARAMS, void* ws, uint64_t ws_bytes, void* stream) {
    const HgtDetWs det = {ws, ws_bytes};
    return typed_colsum_impl(HGT_COLSUM_ARGS, &det, stream);
}
