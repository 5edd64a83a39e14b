// Relation outer products of the backward pass (d relation_msg, d A'; the derivation is in hgt_bwd_update.hip): hgt_relation_outer for
// heads of up to 64 padded columns, hgt_relation_outer_wide for 128 / 256.  One host function behind the four entry points (hgt_det.h).
#include "hgt_det.h"
#include "hgt_edge_common.h"
#include "hgt_split_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Relation outer products:  out[r][h][k][c] += sum_{e of relation r} w_e,h * a[src_e][h][k] * b[dst_e][h][c]
// (d relation_msg with (w, a, b) = (att, V, dagg); d A' with (ds, K, Q)).  A wavefront takes the work items of ONE relation
// (blockIdx.z) inside its slice of the plan's item list (runs of <= 512 sorted edges of one (tile, relation)); lane = (head,
// VEC rows k of the head's block); the b row of the edge is broadcast inside the head's lanes through LDS; the dkp x dkp
// blocks accumulate in registers over ~64 items and are flushed once with atomics.
// ---------------------------------------------------------------------------------------------
// DET (k_det_relation_outer*): the wavefront's blocks are STORED into its own [R][HT][dkp][dkp] slot of `out` (= the workspace;
// slot = the wavefront's slice of the item list, slices without an item of the relation store zeros) instead of added to out.
#define HGT_OUTER_PARAMS                                                                                                             \
    const HgtItem *__restrict__ items, const HgtPlanHeader *__restrict__ hdr, const int32_t *__restrict__ esrc,                        \
        const int32_t *__restrict__ edst, const uint16_t *__restrict__ ertei, const float *__restrict__ w, const float *__restrict__ a, \
        const float *__restrict__ rte_a, const float *__restrict__ b, float *__restrict__ out, int R, int HT, int items_per_wave
#define HGT_OUTER_ARGS items, hdr, esrc, edst, ertei, w, a, rte_a, b, out, R, HT, items_per_wave

template <int VEC, int LPH, bool RTE, bool DET>
__device__ __forceinline__ void relation_outer_body(HGT_OUTER_PARAMS) {
    constexpr int DKP = VEC * LPH, DP = 64 * VEC, H = 64 / LPH;
    __shared__ __attribute__((aligned(16))) float s_b[4][DP + 4 * (64 / LPH)];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hg = blockIdx.y;
    const int rel_sel = blockIdx.z;            // this wavefront only takes the items of ONE relation: one flush per wavefront
    const int64_t ld = (int64_t)HT * DKP;
    const int co = hg * DP;
    const int h = lane / LPH, p = lane % LPH;
    float* bounce = s_b[wib];
    const int n_items = hdr->n_items;
    const int first = (blockIdx.x * 4 + wib) * items_per_wave;
    if (!DET && first >= n_items) return;
    if constexpr (DET) out += (int64_t)(blockIdx.x * 4 + wib) * R * HT * DKP * DKP;
    float acc[VEC][DKP];      // rows k = p*VEC + i of head h, all DKP columns
#pragma unroll
    for (int i = 0; i < VEC; ++i)
#pragma unroll
        for (int c = 0; c < DKP; ++c) acc[i][c] = 0.0f;
    bool any = false;
    for (int ib = first; ib < min(first + items_per_wave, n_items); ib += 64) {
        // 64 item headers at a time (lane i = item ib + i); the matching ones are walked one after the other
        const int my_i = min(ib + lane, n_items - 1);
        const HgtItem mine = items[my_i];
        const bool take = (ib + lane < min(first + items_per_wave, n_items)) && mine.rel == rel_sel;
        unsigned long long todo = __builtin_amdgcn_ballot_w64(take);
        while (todo) {
            const int li_ = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int beg = __builtin_amdgcn_readlane(mine.beg, li_), end = __builtin_amdgcn_readlane(mine.end, li_);
            any = true;
            for (int base = beg; base < end; base += 64) {
                const int nb = min(64, end - base);
                const int li = base + min(lane, nb - 1);
                const int my_src = esrc[li], my_dst = edst[li];
                const int my_rte = RTE ? (int)ertei[li] : 0;
                // UB edges per batch: all their row / weight loads are issued (unconditionally: slots beyond the chunk re-read
                // its last edge) before the first one is consumed -- one memory round trip per batch instead of one per edge
                // (the per-edge form ran 15.7 ms at c2, the whole backward pass 68 ms)
                constexpr int UB = (VEC * DKP <= 128 && !RTE) ? 8 : 4;      // (more would push the kernel past 256 registers = one wavefront per SIMD)
                for (int e0 = 0; e0 < nb; e0 += UB) {
                    float av[UB][VEC], bv[UB][VEC], tv[RTE ? UB : 1][VEC], we[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const int idx = min(e0 + u, nb - 1);
                        const int s = __builtin_amdgcn_readlane(my_src, idx), dd = __builtin_amdgcn_readlane(my_dst, idx);
                        load_vec<VEC>(a + (int64_t)s * ld + co + lane * VEC, av[u]);
                        if constexpr (RTE) {
                            const int ri = __builtin_amdgcn_readlane(my_rte, idx);
                            load_vec<VEC>(rte_a + (int64_t)ri * ld + co + lane * VEC, tv[u]);
                        }
                        load_vec<VEC>(b + (int64_t)dd * ld + co + lane * VEC, bv[u]);
                        we[u] = w[(int64_t)(base + idx) * HT + hg * H + h];
                    }
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        if (e0 + u < nb) {
#pragma unroll
                            for (int i = 0; i < VEC; ++i) {
                                if constexpr (RTE) av[u][i] += tv[u][i];
                                av[u][i] *= we[u];
                            }
                            store_vec_lds<VEC>(bounce + lane * VEC + (lane / LPH) * 4, bv[u]);
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            const float* xb = bounce + h * (DKP + 4);
#pragma unroll
                            for (int c4 = 0; c4 < DKP / 4; ++c4) {
                                const float4 bb = *reinterpret_cast<const float4*>(xb + 4 * c4);
#pragma unroll
                                for (int i = 0; i < VEC; ++i) {
                                    acc[i][4 * c4 + 0] = fmaf(av[u][i], bb.x, acc[i][4 * c4 + 0]);
                                    acc[i][4 * c4 + 1] = fmaf(av[u][i], bb.y, acc[i][4 * c4 + 1]);
                                    acc[i][4 * c4 + 2] = fmaf(av[u][i], bb.z, acc[i][4 * c4 + 2]);
                                    acc[i][4 * c4 + 3] = fmaf(av[u][i], bb.w, acc[i][4 * c4 + 3]);
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                        }
                    }
                }
            }
        }
    }
    if (any || DET) {
        float* o = out + (((int64_t)rel_sel * HT + hg * H + h) * DKP + p * VEC) * DKP;
#pragma unroll
        for (int i = 0; i < VEC; ++i)
#pragma unroll
            for (int c = 0; c < DKP; ++c) {
                if constexpr (DET) o[i * DKP + c] = acc[i][c];
                else unsafeAtomicAdd(&o[i * DKP + c], acc[i][c]);
            }
    }
}
template <int VEC, int LPH, bool RTE>
__global__ __launch_bounds__(256) void k_relation_outer(HGT_OUTER_PARAMS) { relation_outer_body<VEC, LPH, RTE, false>(HGT_OUTER_ARGS); }
template <int VEC, int LPH, bool RTE>
__global__ __launch_bounds__(256) void k_det_relation_outer(HGT_OUTER_PARAMS) { relation_outer_body<VEC, LPH, RTE, true>(HGT_OUTER_ARGS); }

// The same sums on the matrix cores for 32-wide heads (d_k = 32: c2, c3): the outer products of an edge batch are one
// v_mfma_f32_32x32x2_f32 per (head, pair of edges) -- operand A = the two scaled source rows' 32 head columns, B = the two target
// rows' -- exact fp32 products, 256 matrix-core cycles per edge instead of ~550 vector-ALU cycles (128 FMAs per lane, LDS bounce,
// two wave barriers per edge).  The rows of a batch are parked in LDS as [edge][column] (288-float stride: the two edges of a pair
// fall into different bank halves); the 8 head blocks accumulate in 128 registers and are flushed once per wavefront.
template <int VEC, bool RTE, bool DET>
__device__ __forceinline__ void relation_outer_mfma_body(HGT_OUTER_PARAMS) {
    constexpr int DKP = 32, LPH = DKP / VEC, DP = 64 * VEC, H = 64 / LPH, UB = 8, RS = DP + 32;   // RS: LDS row stride in floats
    static_assert(DP % 32 == 0 && H * DKP == DP, "32-wide heads");
    __shared__ __attribute__((aligned(16))) float s_rows[4][2][UB][RS];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hg = blockIdx.y, rel_sel = blockIdx.z;
    const int64_t ld = (int64_t)HT * DKP;
    const int co = hg * DP;
    const int h = lane / LPH;
    float (*sa)[RS] = s_rows[wib][0];
    float (*sb)[RS] = s_rows[wib][1];
    const int n_items = hdr->n_items;
    const int first = (blockIdx.x * 4 + wib) * items_per_wave;
    if (!DET && first >= n_items) return;
    if constexpr (DET) out += (int64_t)(blockIdx.x * 4 + wib) * R * HT * DKP * DKP;
    f32x16 acc[H];
#pragma unroll
    for (int hh = 0; hh < H; ++hh)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[hh][r] = 0.0f;
    bool any = false;
    for (int ib = first; ib < min(first + items_per_wave, n_items); ib += 64) {
        const int my_i = min(ib + lane, n_items - 1);
        const HgtItem mine = items[my_i];
        const bool take = (ib + lane < min(first + items_per_wave, n_items)) && mine.rel == rel_sel;
        unsigned long long todo = __builtin_amdgcn_ballot_w64(take);
        while (todo) {
            const int li_ = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int beg = __builtin_amdgcn_readlane(mine.beg, li_), end = __builtin_amdgcn_readlane(mine.end, li_);
            any = true;
            for (int base = beg; base < end; base += 64) {
                const int nb = min(64, end - base);
                const int li = base + min(lane, nb - 1);
                const int my_src = esrc[li], my_dst = edst[li];
                const int my_rte = RTE ? (int)ertei[li] : 0;
                for (int e0 = 0; e0 < nb; e0 += UB) {
                    float av[UB][VEC], bv[UB][VEC], tv[RTE ? UB : 1][VEC], we[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const int idx = min(e0 + u, nb - 1);
                        const int s = __builtin_amdgcn_readlane(my_src, idx), dd = __builtin_amdgcn_readlane(my_dst, idx);
                        load_vec<VEC>(a + (int64_t)s * ld + co + lane * VEC, av[u]);
                        if constexpr (RTE) {
                            const int ri = __builtin_amdgcn_readlane(my_rte, idx);
                            load_vec<VEC>(rte_a + (int64_t)ri * ld + co + lane * VEC, tv[u]);
                        }
                        load_vec<VEC>(b + (int64_t)dd * ld + co + lane * VEC, bv[u]);
                        we[u] = w[(int64_t)(base + idx) * HT + hg * H + h];
                    }
                    __builtin_amdgcn_wave_barrier();          // the previous batch's operands have been read
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const float sc = (e0 + u < nb) ? we[u] : 0.0f;      // slots beyond the chunk contribute nothing
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            if constexpr (RTE) av[u][i] += tv[u][i];
                            av[u][i] *= sc;
                        }
                        store_vec_lds<VEC>(&sa[u][lane * VEC], av[u]);
                        store_vec_lds<VEC>(&sb[u][lane * VEC], bv[u]);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const int er = lane >> 5, cc = lane & 31;
#pragma unroll
                    for (int hh = 0; hh < H; ++hh)
#pragma unroll
                        for (int pr = 0; pr < UB / 2; ++pr)
                            acc[hh] = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[2 * pr + er][hh * 32 + cc], sb[2 * pr + er][hh * 32 + cc], acc[hh],
                                                                          0, 0, 0);
                }
            }
        }
    }
    if (any || DET) {
        // C layout of a 32 x 32 block: column c = lane & 31, row k = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int hh = 0; hh < H; ++hh) {
            float* o = out + ((int64_t)rel_sel * HT + hg * H + hh) * DKP * DKP;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if constexpr (DET) o[k * DKP + (lane & 31)] = acc[hh][r];
                else unsafeAtomicAdd(&o[k * DKP + (lane & 31)], acc[hh][r]);
            }
        }
    }
}
template <int VEC, bool RTE>
__global__ __launch_bounds__(256, 2) void k_relation_outer_mfma(HGT_OUTER_PARAMS) { relation_outer_mfma_body<VEC, RTE, false>(HGT_OUTER_ARGS); }
template <int VEC, bool RTE>
__global__ __launch_bounds__(256, 2) void k_det_relation_outer_mfma(HGT_OUTER_PARAMS) { relation_outer_mfma_body<VEC, RTE, true>(HGT_OUTER_ARGS); }
using OuterKernel = void (*)(HGT_OUTER_PARAMS);
#undef HGT_OUTER_PARAMS
#undef HGT_OUTER_ARGS

// Heads of 128 and 256 padded columns (hgt_relation_outer_wide): per head the sum is a dkp x dkp GEMM whose reduction dimension is
// the relation's edges -- far past what a wavefront's registers hold, so a WORKGROUP owns one 128 x 128 block of one head of one
// relation (blockIdx.y = (head, row block, column block), blockIdx.z = relation) and its four wavefronts the four 64 x 64 quadrants:
// 2 x 2 v_mfma_f32_32x32x2_f32 accumulators each (exact fp32 products, 64 registers).  The workgroup walks the matching items of
// its slice of the item list; per batch of OW_UB edges its 256 threads gather the 128-column segments of the source rows (+ temporal
// rows), scale them with the edge weight and park them next to the target rows' segments in LDS ([edge][column], stride 160 floats:
// the two edges of an MFMA pair fall into different bank halves), so a segment is read from memory once per block instead of once
// per quadrant.  Two LDS buffers: one barrier per batch; the next batch of the item is fetched while the matrix cores run.
constexpr int OW_UB = 16;             // edges per batch (two per thread and operand)
constexpr int OW_RS = 128 + 32;       // LDS row stride in floats
constexpr int OW_ITEMS_SMALL = 8, OW_ITEMS_LARGE = 64;   // items per workgroup = this x (R + 1): outer_items_per_wave's 2 / 16 x 4

struct OwBatch {                      // one thread's share of a batch: 4 columns of two edges' rows, and the edges' weights
    float4 a[2], t[2], b[2];
    float w[2];
};

#define HGT_OUTER_WIDE_PARAMS                                                                                                        \
    const HgtItem *__restrict__ items, const HgtPlanHeader *__restrict__ hdr, const int32_t *__restrict__ esrc,                        \
        const int32_t *__restrict__ edst, const uint16_t *__restrict__ ertei, const float *__restrict__ w, const float *__restrict__ a, \
        const float *__restrict__ rte_a, const float *__restrict__ b, float *__restrict__ out, int HT, int dkp, int items_per_wg
// DET (k_det_relation_outer_wide): the workgroup's block is STORED into slot blockIdx.x ([gridDim.z][HT][dkp][dkp]) of `out` (= the
// workspace); a slice without an item of the relation stores zeros
template <bool RTE, bool DET>
__device__ __forceinline__ void relation_outer_wide_body(HGT_OUTER_WIDE_PARAMS) {
    __shared__ __attribute__((aligned(16))) float s_rows[2][2][OW_UB][OW_RS];      // [buffer][a | b][edge][column]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nblk_h = dkp / 128;                              // 128-column blocks per head side: 1 or 2
    const int h = blockIdx.y / (nblk_h * nblk_h);
    const int kb = (blockIdx.y / nblk_h) % nblk_h, cb = blockIdx.y % nblk_h;
    const int rel_sel = blockIdx.z;
    const int64_t ld = (int64_t)HT * dkp;
    const int n_items = hdr->n_items;
    const int first = blockIdx.x * items_per_wg;
    if (!DET && first >= n_items) return;
    if constexpr (DET) out += (int64_t)blockIdx.x * gridDim.z * HT * dkp * dkp;
    const int last = min(first + items_per_wg, n_items);
    // gather role: thread = (edge slot u of the batch (and u + 8), 4 columns)
    const int u = tid >> 5, c4 = (tid & 31) * 4;
    const float* a_seg = a + h * dkp + kb * 128 + c4;
    const float* t_seg = RTE ? rte_a + h * dkp + kb * 128 + c4 : nullptr;
    const float* b_seg = b + h * dkp + cb * 128 + c4;
    // matrix-core role: wavefront = quadrant (qr, qc); lane = (edge of the pair, row / column inside a 32-wide tile)
    const int qr = wib >> 1, qc = wib & 1;
    const int er = lane >> 5, cc = lane & 31;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    OwBatch bt;
    auto fetch = [=](int e0, int end) {
        OwBatch n;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = e0 + u + 8 * k;
            const int idx = min(e, end - 1);           // slots beyond the item re-read its last edge with weight 0
            const int s = esrc[idx], dd = edst[idx];
            n.a[k] = *reinterpret_cast<const float4*>(a_seg + (int64_t)s * ld);
            if constexpr (RTE) n.t[k] = *reinterpret_cast<const float4*>(t_seg + (int64_t)ertei[idx] * ld);
            else n.t[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // (never read: a fully written struct stays in registers)
            n.b[k] = *reinterpret_cast<const float4*>(b_seg + (int64_t)dd * ld);
            n.w[k] = e < end ? w[(int64_t)idx * HT + h] : 0.0f;
        }
        return n;
    };
    int buf = 0;
    bool any = false;
    for (int ib = first; ib < last; ib += 64) {
        // 64 item headers at a time (lane i = item ib + i), the same in every wavefront: the loops below are workgroup-uniform
        const HgtItem mine = items[min(ib + lane, n_items - 1)];
        const bool take = (ib + lane < last) && mine.rel == rel_sel;
        unsigned long long todo = __builtin_amdgcn_ballot_w64(take);
        while (todo) {
            const int li_ = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int beg = __builtin_amdgcn_readlane(mine.beg, li_), end = __builtin_amdgcn_readlane(mine.end, li_);
            if (beg >= end) continue;
            any = true;
            bt = fetch(beg, end);
            for (int e0 = beg; e0 < end; e0 += OW_UB) {
                float (*sa)[OW_RS] = s_rows[buf][0];
                float (*sb)[OW_RS] = s_rows[buf][1];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    float4 v = bt.a[k];
                    if constexpr (RTE) { v.x += bt.t[k].x; v.y += bt.t[k].y; v.z += bt.t[k].z; v.w += bt.t[k].w; }
                    v.x *= bt.w[k]; v.y *= bt.w[k]; v.z *= bt.w[k]; v.w *= bt.w[k];
                    *reinterpret_cast<float4*>(&sa[u + 8 * k][c4]) = v;
                    *reinterpret_cast<float4*>(&sb[u + 8 * k][c4]) = bt.b[k];
                }
                // one barrier per batch: this buffer was last read two batches ago, before the previous batch's barrier
                __syncthreads();
                if (e0 + OW_UB < end) bt = fetch(e0 + OW_UB, end);
#pragma unroll
                for (int pr = 0; pr < OW_UB / 2; ++pr) {
                    float fa[2], fb[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        fa[i] = sa[2 * pr + er][qr * 64 + i * 32 + cc];
                        fb[i] = sb[2 * pr + er][qc * 64 + i * 32 + cc];
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
                }
                buf ^= 1;
            }
        }
    }
    if (any || DET) {
        // C layout of a 32 x 32 tile: column c = lane & 31, row k = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        float* o = out + (((int64_t)rel_sel * HT + h) * dkp + kb * 128 + qr * 64) * dkp + cb * 128 + qc * 64;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * er;
                    if constexpr (DET) o[(int64_t)k * dkp + j * 32 + cc] = acc[i][j][r];
                    else unsafeAtomicAdd(&o[(int64_t)k * dkp + j * 32 + cc], acc[i][j][r]);
                }
    }
}
template <bool RTE>
__global__ __launch_bounds__(256, 2) void k_relation_outer_wide(HGT_OUTER_WIDE_PARAMS) {
    relation_outer_wide_body<RTE, false>(items, hdr, esrc, edst, ertei, w, a, rte_a, b, out, HT, dkp, items_per_wg);
}
template <bool RTE>
__global__ __launch_bounds__(256, 2) void k_det_relation_outer_wide(HGT_OUTER_WIDE_PARAMS) {
    relation_outer_wide_body<RTE, true>(items, hdr, esrc, edst, ertei, w, a, rte_a, b, out, HT, dkp, items_per_wg);
}
#undef HGT_OUTER_WIDE_PARAMS

// the atomic or the det kernel, without or with temporal rows
template <class K>
inline K pick_kernel(bool det, bool rte, K atomic_plain, K atomic_rte, K det_plain, K det_rte) {
    return det ? (rte ? det_rte : det_plain) : (rte ? atomic_rte : atomic_plain);
}

// ---- launch geometry: a slot = the slice of `ipw` items of the plan's item list that one wavefront (narrow kernels) / one workgroup
// (wide kernel) walks; the det forms keep one partial per slot
struct OuterPlan { int64_t slots; int ipw; };

// Items per wavefront of the atomic narrow kernels: ~16 items of the selected relation per wavefront (items are ordered (tile,
// relation)): at c2 3 000 wavefronts for 1 024 SIMDs (64 items left the chip with fewer wavefronts than SIMDs) against 25 M flush
// atomics (sampled batches -- a few thousand 16-edge items: 16 (R + 1) items per wavefront left 13 x R wavefronts walking ~250 edges
// each, 565 us per call at c3 (r6 timeline of a training step); 2 (R + 1) there)
inline int outer_items_per_wave(int64_t max_items, int R) { return (max_items < 16384 ? 2 : 16) * (R + 1); }
// Items per workgroup of the atomic wide kernel: the same two regimes x 4 wavefronts (sampled batches: enough workgroups to fill the
// chip; large graphs: fewer 128 x 128 atomic flushes)
inline int outer_wide_items_per_wg(int64_t max_items, int R) { return (max_items < 16384 ? OW_ITEMS_SMALL : OW_ITEMS_LARGE) * (R + 1); }

inline OuterPlan outer_plan(bool wide, int64_t max_items, int R) {
    const int ipw = wide ? outer_wide_items_per_wg(max_items, R) : outer_items_per_wave(max_items, R);
    return {(max_items + ipw - 1) / ipw, ipw};
}
// det: as many slots as the atomic form has, inside a budget of max(DET_FLOOR, 1/4 of the bytes of Q|K|V) for the [R][H][dkp][dkp] partials
inline OuterPlan det_outer_plan(bool wide, int64_t N, int64_t max_items, int R, int H, int dkp) {
    const uint64_t slot_floats = (uint64_t)R * H * dkp * dkp;
    const uint64_t budget = max(DET_FLOOR, (uint64_t)N * H * dkp * 4 * 3 / 4);
    const OuterPlan a = outer_plan(wide, max_items, R);
    // (the narrow kernels launch whole workgroups of four wavefronts = four slots: four is the least they take, also where four
    //  partials pass the budget -- 4 R H dkp^2 floats, dkp <= 64: more than DET_FLOOR only from R H > 512 on)
    int64_t s = det_fit_slots(max((int64_t)1, a.slots) + (wide ? 0 : 3), slot_floats, budget);
    if (!wide) s = max((int64_t)4, s / 4 * 4);
    const int64_t ipw = max((int64_t)a.ipw, (max_items + s - 1) / s);
    const int64_t used = max((int64_t)1, (max_items + ipw - 1) / ipw);
    return {wide ? used : (used + 3) / 4 * 4, (int)ipw};
}

// Lanes of the narrow kernels: the per-lane accumulator block is VEC x DKP floats -- head groups are split (a head over twice the
// lanes, half the rows per lane: head_split_for, the rule of the forward's kernels) until it fits 256 registers
struct OuterLanes { int vec, lph; };
inline OuterLanes outer_lane_split(int H, int dk_pad) {
    const int lph = 64 / H, vec = dk_pad / lph, s = head_split_for(vec, lph, dk_pad);
    return {vec / s, lph * s};
}

template <int VEC, int LPH>
struct LaunchOuter {
    // p: items per wavefront and wavefronts; det: `out` = the workspace (one slot per wavefront)
    static int run(const HgtPlanView& pv, const float* w, const float* a, const float* rte_a, const float* b, float* out, int R, int HT,
                   hipStream_t stream, OuterPlan p, bool det) {
        if constexpr (VEC * LPH * VEC <= 128 && VEC * LPH >= 4) {
            OuterKernel kernel = pick_kernel(det, rte_a != nullptr, k_relation_outer<VEC, LPH, false>, k_relation_outer<VEC, LPH, true>,
                                             k_det_relation_outer<VEC, LPH, false>, k_det_relation_outer<VEC, LPH, true>);
            if constexpr (VEC * LPH == 32 && VEC <= 4)          // 32-wide heads: matrix-core form (the library keeps both, as it always has)
                kernel = pick_kernel(det, rte_a != nullptr, k_relation_outer_mfma<VEC, false>, k_relation_outer_mfma<VEC, true>,
                                     k_det_relation_outer_mfma<VEC, false>, k_det_relation_outer_mfma<VEC, true>);
            dim3 grid(nblk(p.slots, 4), (unsigned)(HT / (64 / LPH)), (unsigned)R);
            kernel<<<grid, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, w, a, rte_a, b, out, R, HT, p.ipw);
            return HGT_OK;
        } else {
            return HGT_ERR_UNSUPPORTED;
        }
    }
};

// ---- host side: one function behind hgt_relation_outer[_wide][_det]
#define HGT_OUTER_HOST_PARAMS                                                                                                       \
    const void *plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad, const float *weights,                  \
        const float *a_src, const float *rte_a, const float *b_dst, float *out
#define HGT_OUTER_HOST_ARGS plan, N, E, T, R, H, dk_pad, weights, a_src, rte_a, b_dst, out

// what the sizes must be (narrow: a head takes 64 / H lanes with dk_pad / (64 / H) columns each)
int outer_shape_check(bool wide, int32_t R, int32_t H, int32_t dk_pad) {
    if (R <= 0 || H <= 0 || dk_pad <= 0) return HGT_ERR_INVALID_ARG;
    if (wide) return dk_pad == 128 || dk_pad == 256 ? HGT_OK : HGT_ERR_UNSUPPORTED;
    return 64 % H == 0 && dk_pad % (64 / H) == 0 ? HGT_OK : HGT_ERR_INVALID_ARG;
}

// hgt_relation_outer_det_bytes / hgt_relation_outer_wide_det_bytes
int outer_det_bytes(bool wide, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad, uint64_t* out) {
    if (!out || N < 0 || E < 0 || T <= 0) return HGT_ERR_INVALID_ARG;
    if (int rc = outer_shape_check(wide, R, H, dk_pad)) return rc;
    *out = E == 0 ? 0 : det_ws_floats(det_outer_plan(wide, N, hgt_plan_layout(N, E, T, R).max_items, R, H, dk_pad).slots,
                                      (uint64_t)R * H * dk_pad * dk_pad) * 4;
    return HGT_OK;
}

// det == NULL: += into the caller's buffer, a relation without edges stays untouched; det: out overwritten.  rte_a optional.
// wide: heads of 128 / 256 padded columns, every other dk_pad is HGT_ERR_UNSUPPORTED there and launches nothing -- the narrow form
// keeps the heads of up to 64 columns.
int relation_outer_impl(bool wide, HGT_OUTER_HOST_PARAMS, const HgtDetWs* det, void* stream) {
    if (!plan || !a_src || !b_dst || !out || (E > 0 && !weights)) return HGT_ERR_INVALID_ARG;
    // hgt_relation_outer answers as it always has (tests/test_backward_args.py): it never looks at n_relations, and on an empty graph
    // it returns HGT_OK once 64 % H == 0 and dk_pad > 0, before dk_pad % (64 / H) is looked at
    const bool lenient = !wide && !det;
    if (lenient && E == 0 && dk_pad > 0 && outer_shape_check(false, 1, H, 64) == HGT_OK) return HGT_OK;
    int rc = outer_shape_check(wide, lenient ? 1 : R, H, dk_pad);
    if (rc != HGT_OK) return rc;
    int64_t blocks = 0;      // wide: the 128 x 128 blocks of all heads = grid.y
    if (wide) {
        if ((((uintptr_t)a_src | (uintptr_t)b_dst | (uintptr_t)rte_a) & 15) != 0) return HGT_ERR_INVALID_ARG;      // 16-byte row loads
        blocks = (int64_t)H * (dk_pad / 128) * (dk_pad / 128);
        if (blocks > 65535 || R > 65535) return HGT_ERR_TOO_LARGE;
    }
    if (det) {
        uint64_t need = 0;
        rc = outer_det_bytes(wide, N, E, T, R, H, dk_pad, &need);
        if (rc == HGT_OK) rc = det_ws_check(*det, need);
        if (rc != HGT_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t elems = (int64_t)R * H * dk_pad * dk_pad;
    if (E == 0) {
        if (!det) return HGT_OK;
        (void)hipMemsetAsync(out, 0, (size_t)elems * 4, st);
        HGT_CHECK_LAUNCH();
        return HGT_OK;
    }
    HgtPlanView pv = hgt_plan_view(plan, N, E, T, R);
    const OuterPlan p = det ? det_outer_plan(wide, N, pv.L.max_items, R, H, dk_pad) : outer_plan(wide, pv.L.max_items, R);
    float* part = det ? (float*)det->ptr : out;      // det: one [R][H][dk_pad][dk_pad] partial per slot, then the segment sums
    if (wide) {
        auto* kernel = pick_kernel(det != nullptr, rte_a != nullptr, k_relation_outer_wide<false>, k_relation_outer_wide<true>,
                                   k_det_relation_outer_wide<false>, k_det_relation_outer_wide<true>);
        kernel<<<dim3((unsigned)p.slots, (unsigned)blocks, (unsigned)R), 256, 0, st>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, weights,
                                                                                     a_src, rte_a, b_dst, part, (int)H, (int)dk_pad, p.ipw);
    } else {
        const OuterLanes l = outer_lane_split(H, dk_pad);
        rc = dispatch_layout<LaunchOuter>(l.vec, l.lph, pv, weights, a_src, rte_a, b_dst, part, (int)R, (int)H, st, p, det != nullptr);
        if (rc != HGT_OK) return rc;
    }
    if (det) det_reduce(part, p.slots, elems, elems, part + p.slots * elems, out, elems, elems, st);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

}  // namespace

extern "C" int hgt_relation_outer_det_bytes(int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad, uint64_t* out) {
    return outer_det_bytes(false, N, E, T, R, H, dk_pad, out);
}
extern "C" int hgt_relation_outer_wide_det_bytes(int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad, uint64_t* out) {
    return outer_det_bytes(true, N, E, T, R, H, dk_pad, out);
}
extern "C" int hgt_relation_outer(HGT_OUTER_HOST_PARAMS, void* stream) {
    return relation_outer_impl(false, HGT_OUTER_HOST_ARGS, nullptr, stream);
}
extern "C" int hgt_relation_outer_det(HGT_OUTER_HOST_PARAMS, void* ws, uint64_t ws_bytes, void* stream) {
    const HgtDetWs det = {ws, ws_bytes};
    return relation_outer_impl(false, HGT_OUTER_HOST_ARGS, &det, stream);
}
// heads of 128 / 256 padded columns (ABI 8)
extern "C" int hgt_relation_outer_wide(HGT_OUTER_HOST_PARAMS, void* stream) {
    return relation_outer_impl(true, HGT_OUTER_HOST_ARGS, nullptr, stream);
}
extern "C" int hgt_relation_outer_wide_det(HGT_OUTER_HOST_PARAMS, void* ws, uint64_t ws_bytes, void* stream) {
    const HgtDetWs det = {ws, ws_bytes};
    return relation_outer_impl(true, HGT_OUTER_HOST_ARGS, &det, stream);
}
