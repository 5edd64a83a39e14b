// Attention logits (conv.py:98-99,104) with the relation transform applied to the SOURCE operand, per edge, on the matrix cores.
//
//     s_e,h = < A'[r,h] q_i,h , k_j,h > = < q_i,h , A'[r,h]^T k_j,h >              (hgt_edge_logits.hip: algebra, A' = att_t)
//
// k_edge_logits applies A' to q once per (target, relation) segment on the vector ALU.  On a graph with short segments (the
// benchmark: 1.75 edges per segment) that is H 32 32 FMAs per 1.75 edges next to 256 for the dots, and every change of target
// is a dependent branch with an LDS bounce.  Here the transform goes to the K row instead: every edge of a work item has the same
// relation, so 32 consecutive edges are the 32 columns of ONE dense product per head,
//     K~^T (32 outputs x 32 edges) = M_{r,h} (32 x 32) . K_h^T (32 x 32 edges),      v_mfma_f32_32x32x16_f16, two k-steps,
// with the edge on the lane: no segments, no target groups, no branch, no LDS.  Lane l is edge l & 31 of the batch, half l >> 5.
// The row and k orders of M are chosen (hgt_kside_map.h) so that the lane supplies columns 16 half .. + 15 of the head's 128-byte
// line of K[src] and receives outputs 16 half .. + 15, which it dots with the same 64 bytes of Q[dst]: four 16-byte loads each per
// head, one cross-half add, and the lane holds the H logits of its edge (lanes 0-31 store them: a full batch is 32 H floats in a row).
//
// Precision: fp16 hi / lo split, three products (lo hi + hi lo + hi hi), for both split precisions.  Every scale is a power of two
// and exact: the K row per (row, head) -- maximum -> [2^14, 2^15) --, M per (relation, head) at pack time, q per (row, head) ->
// [1, 4).  Each is uniform over a head's dot, so the three exponents are undone by ONE ldexp of the finished dot: no fp16 operand
// overflows or is flushed whatever the magnitudes, the fp32 accumulators stay below 2^36, and the logit is finite whenever its fp32
// value is.
//
// Work: a wavefront takes min(H, 4) heads of one work item for all its batches (at H = 8 two wavefronts share an item) and keeps the
// image of its heads in registers (16 per head).  The steps are the (batch, head) pairs in order.
//
// Gather (default): the K and Q pieces of a step arrive by LDS-DMA in whole 128-byte head lines -- one instruction fetches 8 edges x
// one line, lanes 8 r .. 8 r + 7 the eight 16-byte chunks of edge 8 piece + r, four instructions for K and four for Q -- into a ring
// of two 8 KB slots that is private to the wavefront (no workgroup barrier), and the lane reads its 64 + 64 bytes back with eight
// conflict-free ds_read_b128 (maps: hgt_kside_map.h).  A slot is refilled with the step two ahead as soon as its reads have returned
// (lgkmcnt), in front of the step's arithmetic; a step's reads follow a counted vmcnt that leaves the younger step in flight:
// two steps = 16 KB of rows in flight per wavefront, two wavefronts per SIMD (128 KB of LDS per CU), no row buffers in registers.
// The edge ids of the batch after next are the loop's only register loads; they are issued, like the DMAs, where hipcc does not
// count them (it would drain every DMA at their use) and retired by the same counted wait.  Every request is unconditional and of
// fixed size (indices clamped to the item), see hgt_edge_logits.hip.
//
// Lane gather (HGT_FLAG_KSIDE_LANE_GATHER, kept for A/B runs and as the bit-identity reference of the form above; to be retired):
// every lane loads its own 16-byte pieces into min(H, 4) row buffers, the pieces of the step three ahead requested before the
// current one is consumed -- 24 KB in flight, but 64 separate 64-byte sectors per load instruction, which binds the kernel to the
// texture-address units (profiles/kside_logits_*).  Same arithmetic, same logits bit for bit.
#include "hgt_edge_common.h"
#include "hgt_split_common.h"
#include "hgt_kside_map.h"

namespace {

typedef unsigned hgt_u32x2 __attribute__((ext_vector_type(2)));

// the value of the lower and of the upper half's lane (l & 31), in every lane: op(lo, up) is the same in both halves, bit for bit
__device__ __forceinline__ void half_pair(unsigned x, unsigned& lo, unsigned& up) {
#if __has_builtin(__builtin_amdgcn_permlane32_swap)
    const hgt_u32x2 r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    lo = r[0];
    up = r[1];
#else
    const unsigned o = (unsigned)__shfl_xor((int)x, 32);
    const bool upper = (threadIdx.x & 32) != 0;
    lo = upper ? o : x;
    up = upper ? x : o;
#endif
}
__device__ __forceinline__ unsigned half_max_bits(unsigned x) {
    unsigned a, b;
    half_pair(x, a, b);
    return max(a, b);
}
__device__ __forceinline__ float half_sum(float x) {
    unsigned a, b;
    half_pair(__builtin_bit_cast(unsigned, x), a, b);
    return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}

// bits of max |v| over a lane's 16 floats, on the raw bits (a float maximum would first canonicalise every loaded operand): the
// unsigned maximum is the largest negative magnitude if there is a negative value, the signed one the largest positive value if
// there is a positive one, and each falls back to the other's answer otherwise -- the larger magnitude of the two is the maximum
__device__ __forceinline__ unsigned abs_bits16(const float4 (&v)[4]) {
    unsigned mu = 0u;
    int mi = (int)0x80000000u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned x = __builtin_bit_cast(unsigned, v[i].x), y = __builtin_bit_cast(unsigned, v[i].y);
        const unsigned z = __builtin_bit_cast(unsigned, v[i].z), w = __builtin_bit_cast(unsigned, v[i].w);
        mu = max(max(mu, x), y);
        mu = max(max(mu, z), w);
        mi = max(max(mi, (int)x), (int)y);
        mi = max(max(mi, (int)z), (int)w);
    }
    return max(mu & 0x7fffffffu, (unsigned)mi & 0x7fffffffu);
}

// biased exponent of a maximum, clamped so that 2^(141 - e) -- the scale that takes the maximum into [2^14, 2^15) -- is a normal
// float (rows below 2^-113 keep the largest scale: their values stay representable, above fp16's subnormal floor; infinities clamp)
__device__ __forceinline__ int kside_exp(unsigned max_abs_bits) {
    const int e = (int)(max_abs_bits >> 23);
    return e < 14 ? 14 : (e > 254 ? 254 : e);
}
__device__ __forceinline__ float kside_scale(int e) { return __builtin_bit_cast(float, (unsigned)(268 - e) << 23); }

// M_{r,h} = the head's block of att_t, scaled, split and laid out as the A operands of the kernel: one workgroup per (relation, head)
__global__ __launch_bounds__(256) void k_relation_kside_pack(const float* __restrict__ attT, int n_rh, unsigned short* __restrict__ img) {
    __shared__ unsigned s_m[4];
    const int rh = blockIdx.x, t = threadIdx.x;
    const float* blk = attT + (int64_t)rh * HGT_KSIDE_DK * HGT_KSIDE_DK;
    unsigned m = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) m = max(m, __builtin_bit_cast(unsigned, fabsf(blk[t + 256 * q])));
    m = wave_max_bits(m);
    if ((t & 63) == 0) s_m[t >> 6] = m;
    __syncthreads();
    m = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
    const int e = kside_exp(m);
    const float scale = kside_scale(e);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = t + 256 * q;                      // (k-step, lane, j) of the block
        const int j = p & 7, lane = (p >> 3) & 63, s = p >> 9;
        const float v = blk[hgt_kside_image_out(lane) * HGT_KSIDE_DK + hgt_kside_image_k(s, lane, j)];
        unsigned short hi, lo;
        split1_t<true>(v, scale, hi, lo);
        img[hgt_kside_image_index(rh, s, 0, lane, j)] = hi;
        img[hgt_kside_image_index(rh, s, 1, lane, j)] = lo;
    }
    if (t == 0) reinterpret_cast<int*>(img + (int64_t)n_rh * HGT_KSIDE_BLOCK_ELEMS)[rh] = e - 141;
}

typedef unsigned hgt_u32x4 __attribute__((ext_vector_type(4)));

struct KsideRows {   // a lane's 64 bytes of K[src] and of Q[dst] for one head
    float4 k[4], q[4];
};

typedef __amdgpu_buffer_rsrc_t kside_rsrc;

// Q and K are read through buffer descriptors: the lane offsets are 32-bit by construction (coverage: every row below 4 GiB), a
// request behind the table returns zeros, and -- unlike a plain vector load, which the optimiser splits per element and moves to
// the first use of each -- a buffer load stays where the pipeline issues it.
__device__ __forceinline__ kside_rsrc kside_table(const float* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 kside_load16(kside_rsrc t, unsigned off) {
    const hgt_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(t, (int)off, 0, 0);
    return __builtin_bit_cast(float4, v);
}

template <int H>
__device__ __forceinline__ void kside_issue(kside_rsrc K, kside_rsrc Q, unsigned koff, unsigned qoff, int h, KsideRows& b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) b.k[i] = kside_load16(K, koff + h * 128 + 16 * i);
#pragma unroll
    for (int i = 0; i < 4; ++i) b.q[i] = kside_load16(Q, qoff + h * 128 + 16 * i);
}

// ---- gather through LDS (hgt_kside_map.h: gather maps) ----
constexpr unsigned KSIDE_PIECE = 1024;                    // bytes one LDS-DMA instruction writes: 8 edges x a 128-byte head line
constexpr unsigned KSIDE_SIDE = 4 * KSIDE_PIECE;          // the K (or Q) head lines of a batch of 32 edges
constexpr unsigned KSIDE_SLOT = 2 * KSIDE_SIDE;           // a step: K pieces, then Q pieces
constexpr unsigned KSIDE_RING = 2;                        // slots per wavefront
constexpr unsigned KSIDE_WAVE_LDS = KSIDE_RING * KSIDE_SLOT;

// the same descriptor as kside_table, as four scalar words for the LDS-DMA statements
__device__ __forceinline__ hgt_u32x4 kside_table_words(const float* p, unsigned bytes) {
    const uint64_t a = (uint64_t)(uintptr_t)p;
    const hgt_u32x4 r = {(unsigned)a, (unsigned)(a >> 32) & 0xffffu, bytes, 0x00020000u};
    return r;
}
// The four pieces of one side of a step: 64 lanes x 16 B each from table[voff[p] + soff] to LDS [lds_dst + 1024 p + 16 lane].  M0 (the
// LDS destination; compiler-reserved) is written and restored inside the statement; soff goes into the scalar offset, which -- unlike
// the instruction's immediate -- moves the source only.  The opening s_nop, with the three instructions in front of the first load,
// covers the wait states of a scalar operand that a vector instruction (readfirstlane) wrote.  Not counted by hipcc: kside_wait_vm.
__device__ __forceinline__ void kside_dma4(hgt_u32x4 table, const unsigned (&voff)[4], unsigned soff, unsigned lds_dst) {
    unsigned keep;
    asm volatile(
        "s_nop 1\n\ts_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %6\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %5, %7 offen lds\n\t"
        "s_add_u32 m0, %6, 0x400\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %5, %7 offen lds\n\t"
        "s_add_u32 m0, %6, 0x800\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %5, %7 offen lds\n\t"
        "s_add_u32 m0, %6, 0xc00\n\ts_nop 0\n\tbuffer_load_dwordx4 %4, %5, %7 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "s"(table), "s"(lds_dst), "s"(soff)
        : "memory", "scc");
}
static_assert(KSIDE_PIECE == 0x400, "the piece stride written into kside_dma4");
constexpr int KSIDE_STEP_DMAS = 8;      // LDS-DMA instructions of a step: the count every wait below leaves in flight
// all but the youngest step's DMAs have landed (vector memory operations retire in order)
__device__ __forceinline__ void kside_wait_vm() { asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }
// ... and with them the edge ids requested by kside_ids_request in front of that youngest step
__device__ __forceinline__ void kside_wait_vm_ids(int& s, int& d) { asm volatile("s_waitcnt vmcnt(8)" : "+v"(s), "+v"(d) : : "memory"); }
__device__ __forceinline__ void kside_ids_request(const int32_t* ps, const int32_t* pd, int& s, int& d) {
    asm volatile("global_load_dword %0, %2, off\n\tglobal_load_dword %1, %3, off" : "=&v"(s), "=&v"(d) : "v"(ps), "v"(pd) : "memory");
}
__device__ __forceinline__ void kside_wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// per-lane byte offsets of a batch's eight pieces (K 0-3, Q 4-7) from the edge ids the lane holds for edge lane & 31
__device__ __forceinline__ void kside_piece_offsets(int s, int d, const int (&bp)[4], const unsigned (&cp)[4], unsigned rowb, unsigned (&off)[8]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        off[p] = (unsigned)__builtin_amdgcn_ds_bpermute(bp[p], s) * rowb + cp[p];
        off[4 + p] = (unsigned)__builtin_amdgcn_ds_bpermute(bp[p], d) * rowb + cp[p];
    }
}

// one head of one batch: split the K piece, six MFMAs, dot with the Q piece, undo the three scales
__device__ __forceinline__ float kside_head(const KsideRows& b, const hgt_f16x8 (&ah)[2], const hgt_f16x8 (&al)[2], int ea) {
    const int ek = kside_exp(half_max_bits(abs_bits16(b.k)));
    const float ks = kside_scale(ek);
    hgt_f16x8 kh[2], kl[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        static_assert(hgt_kside_k_col(1, 0, 0) == 8 && hgt_kside_k_col(0, 1, 0) == 16, "k-step s takes floats 8 s .. 8 s + 7 of the lane's piece");
        uint4 hi, lo;
        split2_f16(b.k[2 * s].x * ks, b.k[2 * s].y * ks, hi.x, lo.x);
        split2_f16(b.k[2 * s].z * ks, b.k[2 * s].w * ks, hi.y, lo.y);
        split2_f16(b.k[2 * s + 1].x * ks, b.k[2 * s + 1].y * ks, hi.z, lo.z);
        split2_f16(b.k[2 * s + 1].z * ks, b.k[2 * s + 1].w * ks, hi.w, lo.w);
        kh[s] = __builtin_bit_cast(hgt_f16x8, hi);
        kl[s] = __builtin_bit_cast(hgt_f16x8, lo);
    }
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[0], kh[0], acc, 0, 0, 0);      // the small terms first
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[1], kh[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[0], kl[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[1], kl[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[0], kh[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[1], kh[1], acc, 0, 0, 0);
    // q -> [1, 4): the products with the accumulators (below 2^36) cannot overflow
    int eq = (int)(half_max_bits(abs_bits16(b.q)) >> 23);
    eq = eq < 1 ? 1 : (eq > 253 ? 253 : eq);
    const float qs = __builtin_bit_cast(float, (unsigned)(254 - eq) << 23);
    static_assert(hgt_kside_c_out(1, 5) == 21, "register reg of the accumulator is output 16 half + reg: the lane's own Q piece");
    const hgt_f32x2 qs2 = {qs, qs};
    hgt_f32x2 d = {0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const hgt_f32x2 q0 = {b.q[i].x, b.q[i].y}, q1 = {b.q[i].z, b.q[i].w};
        const hgt_f32x2 a0 = {acc[4 * i], acc[4 * i + 1]}, a1 = {acc[4 * i + 2], acc[4 * i + 3]};
        d = __builtin_elementwise_fma(q0 * qs2, a0, d);
        d = __builtin_elementwise_fma(q1 * qs2, a1, d);
    }
    const float d0 = d[0], d1 = d[1];
    return ldexpf(half_sum(d0 + d1), (eq - 127) + (ek - 141) + ea);
}

// HW heads per wavefront: a wavefront takes HW = min(H, 4) heads of its item for all the item's batches, so at H = 8 two wavefronts
// share an item (each reads its 512-byte half of every row, stores its four logits of every edge) and a workgroup takes 4 H / 8 ... 4
// items.  The image of HW heads is 16 HW registers.  LANE: the per-lane gather into HW row buffers (see the head of the file).
template <int H, bool LANE>
__global__ __launch_bounds__(256, 2) void k_edge_logits_kside(
    const HgtItem* __restrict__ items, const HgtPlanHeader* __restrict__ hdr, const int32_t* __restrict__ esrc,
    const int32_t* __restrict__ edst, const float* __restrict__ Qp, const float* __restrict__ Kp, unsigned table_bytes,
    const unsigned short* __restrict__ img, float* __restrict__ logits, int R, int item_lo, int item_hi, int items_cap) {
    static_assert(H == 2 || H == 4 || H == 8, "one head group of 32-column heads");
    constexpr int HW = H < 4 ? H : 4, WPI = H / HW;      // heads per wavefront, wavefronts per item
    constexpr unsigned ROWB = H * 128;                   // bytes of a Q / K row
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = item_lo + hgt_item_block() * (4 / WPI) + wib / WPI;      // (XCD-aware item order: hgt_edge_common.h)
    const int h0 = (wib % WPI) * HW;                         // first head of this wavefront
    const HgtItem it = items[min(item, items_cap - 1)];      // (requested together with the header's item count: see k_edge_logits)
    if (item >= (item_hi >= 0 ? item_hi : hdr->n_items)) return;      // (item_lo, item_hi): the items of a target block, or (0, -1)
    const int beg = __builtin_amdgcn_readfirstlane(it.beg), end = __builtin_amdgcn_readfirstlane(it.end);
    const int rel = __builtin_amdgcn_readfirstlane(it.rel);
    if (beg >= end) return;
    if (rel >= R) {   // edges no meta relation claims: logit 0 (conv.py:68)
        if (h0 == 0)
            for (int64_t i = (int64_t)beg * H + lane; i < (int64_t)end * H; i += 64) logits[i] = 0.0f;
        return;
    }
    const int el = lane & 31, half = lane >> 5;

    // the relation's image: A operands of this wavefront's heads, and the exponents that undo their scales
    hgt_f16x8 ah[HW][2], al[HW][2];
    {
        const uint4* ip = reinterpret_cast<const uint4*>(img) + ((int64_t)rel * H + h0) * 256 + lane;
#pragma unroll
        for (int h = 0; h < HW; ++h)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                ah[h][s] = __builtin_bit_cast(hgt_f16x8, ip[((h * 2 + s) * 2 + 0) * 64]);
                al[h][s] = __builtin_bit_cast(hgt_f16x8, ip[((h * 2 + s) * 2 + 1) * 64]);
            }
    }
    const int* eap = reinterpret_cast<const int*>(img + (int64_t)R * H * HGT_KSIDE_BLOCK_ELEMS) + rel * H + h0;
    int ea[HW];
#pragma unroll
    for (int h = 0; h < HW; ++h) ea[h] = eap[h];

    if constexpr (LANE) {
        // Software pipeline over the steps (batch of 32 edges, head): buffer h holds head h; step (b, h) first requests the pieces of the
        // step HW - 1 ahead -- (b, HW - 1) at h = 0, (b + 1, h - 1) otherwise -- into the buffer the previous step released.  The edge
        // indices run one batch further ahead.  Indices are clamped to the item, so the requests behind its end re-read its last edge.
        const kside_rsrc K = kside_table(Kp, table_bytes), Q = kside_table(Qp, table_bytes);
        const unsigned lo = (unsigned)half * 64u + (unsigned)h0 * 128u;
        int li = min(beg + el, end - 1);
        unsigned koff = (unsigned)esrc[li] * ROWB + lo, qoff = (unsigned)edst[li] * ROWB + lo;
        li = min(beg + 32 + el, end - 1);
        unsigned koff_n = (unsigned)esrc[li] * ROWB + lo, qoff_n = (unsigned)edst[li] * ROWB + lo;
        KsideRows buf[HW];
#pragma unroll
        for (int h = 0; h < HW - 1; ++h) kside_issue<H>(K, Q, koff, qoff, h, buf[h]);
        li = min(beg + 64 + el, end - 1);
        int s2 = esrc[li], d2 = edst[li];
        for (int base = beg; base < end; base += 32) {
            float lg[HW];
#pragma unroll
            for (int h = 0; h < HW; ++h) {
                // (the barriers pin every request in front of the arithmetic it overlaps: left free, the scheduler moves the loads to
                //  where their registers are needed and one step's pieces are in flight instead of HW - 1)
                if (h == 0) kside_issue<H>(K, Q, koff, qoff, HW - 1, buf[HW - 1]);
                else kside_issue<H>(K, Q, koff_n, qoff_n, h - 1, buf[h - 1]);
                __builtin_amdgcn_sched_barrier(0);
                lg[h] = kside_head(buf[h], ah[h], al[h], ea[h]);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (half == 0 && base + el < end) {
                float* o = logits + (int64_t)(base + el) * H + h0;
                if constexpr (HW == 2) *reinterpret_cast<float2*>(o) = make_float2(lg[0], lg[1]);
                else *reinterpret_cast<float4*>(o) = make_float4(lg[0], lg[1], lg[2], lg[3]);
            }
            koff = koff_n;
            qoff = qoff_n;
            koff_n = (unsigned)s2 * ROWB + lo;
            qoff_n = (unsigned)d2 * ROWB + lo;
            li = min(base + 96 + el, end - 1);
            s2 = esrc[li];
            d2 = edst[li];
        }
    } else {
        // Ring of two slots per wavefront: step t = (batch, head h) lives in slot h & 1 (HW is even).  Step t: wait until only the
        // DMAs of step t + 1 are in flight, read the slot, wait for the reads, refill the slot with step t + 2 -- head h + 2 of this
        // batch or head h + 2 - HW of the next --, then the arithmetic of step t.  off_c / off_n are the piece offsets of this and of
        // the next batch; the edge ids of the batch after next are requested in front of step 0's refill and are therefore retired by
        // step 1's wait (older than the only step it leaves in flight).  The logit store between two batches only makes a wait stricter.
        static_assert(HW % 2 == 0 && KSIDE_RING == 2 && KSIDE_STEP_DMAS == 8, "slot of a step = its head & 1; eight DMAs per step");
        __shared__ __attribute__((aligned(1024))) unsigned char ring[4 * KSIDE_WAVE_LDS];
        const unsigned lds_wave = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)ring) +
                                  (unsigned)wib * KSIDE_WAVE_LDS;
        const unsigned char* rd = ring + (unsigned)wib * KSIDE_WAVE_LDS;
        const hgt_u32x4 K = kside_table_words(Kp, table_bytes), Q = kside_table_words(Qp, table_bytes);
        unsigned cp[4], ra[4];      // source byte of the lane's chunk in its edge's row (DMA side), LDS byte of read i (read side)
        int bp[4];                  // the lane that holds the edge id of the lane's DMA row, as a ds_bpermute address
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            cp[p] = (unsigned)h0 * 128u + 16u * (unsigned)hgt_kside_dma_chunk(p, lane);
            bp[p] = 4 * hgt_kside_dma_edge(p, lane);
            ra[p] = (unsigned)hgt_kside_read_offset(lane, p);
        }
        unsigned off_c[8], off_n[8];
        int li = min(beg + el, end - 1);
        kside_piece_offsets(esrc[li], edst[li], bp, cp, ROWB, off_c);
        li = min(beg + 32 + el, end - 1);
        kside_piece_offsets(esrc[li], edst[li], bp, cp, ROWB, off_n);
        // (every load hipcc counts is consumed in front of the first DMA: its own waits stay out of the loop)
#pragma unroll
        for (int h = 0; h < HW; ++h)
#pragma unroll
            for (int s = 0; s < 2; ++s) asm volatile("" : "+v"(ah[h][s]), "+v"(al[h][s]));
#pragma unroll
        for (int h = 0; h < HW; ++h) asm volatile("" : "+v"(ea[h]));
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(off_c[i]), "+v"(off_n[i]));
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            kside_dma4(K, reinterpret_cast<const unsigned(&)[4]>(off_c[0]), h * 128u, lds_wave + h * KSIDE_SLOT);
            kside_dma4(Q, reinterpret_cast<const unsigned(&)[4]>(off_c[4]), h * 128u, lds_wave + h * KSIDE_SLOT + KSIDE_SIDE);
        }
        int s2 = 0, d2 = 0;
        for (int base = beg; base < end; base += 32) {
            float lg[HW];
#pragma unroll
            for (int h = 0; h < HW; ++h) {
                const unsigned slot = (h & 1) * KSIDE_SLOT;
                if (h == 1) kside_wait_vm_ids(s2, d2);
                else kside_wait_vm();
                KsideRows b;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    b.k[i] = *reinterpret_cast<const float4*>(rd + slot + ra[i]);
                    b.q[i] = *reinterpret_cast<const float4*>(rd + slot + KSIDE_SIDE + ra[i]);
                }
                kside_wait_lds();
                if (h == 0) {
                    li = min(base + 64 + el, end - 1);
                    kside_ids_request(esrc + li, edst + li, s2, d2);
                }
                const bool same = h + 2 < HW;      // the step two ahead: in this batch, or in the next
                const unsigned hn = (same ? h + 2 : h + 2 - HW) * 128u;
                kside_dma4(K, reinterpret_cast<const unsigned(&)[4]>(same ? off_c[0] : off_n[0]), hn, lds_wave + slot);
                kside_dma4(Q, reinterpret_cast<const unsigned(&)[4]>(same ? off_c[4] : off_n[4]), hn, lds_wave + slot + KSIDE_SIDE);
                __builtin_amdgcn_sched_barrier(0);
                lg[h] = kside_head(b, ah[h], al[h], ea[h]);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (half == 0 && base + el < end) {
                float* o = logits + (int64_t)(base + el) * H + h0;
                if constexpr (HW == 2) *reinterpret_cast<float2*>(o) = make_float2(lg[0], lg[1]);
                else *reinterpret_cast<float4*>(o) = make_float4(lg[0], lg[1], lg[2], lg[3]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) off_c[i] = off_n[i];
            kside_piece_offsets(s2, d2, bp, cp, ROWB, off_n);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the two steps requested behind the item's end: no DMA outlives the wavefront
    }
}

template <int H>
static void launch_kside(const HgtPlanView& pv, const float* Q, const float* K, unsigned table_bytes, const unsigned short* img, float* logits, int R,
                         int item_lo, int item_hi, bool lane_gather, hipStream_t stream) {
    constexpr int IPW = H == 8 ? 2 : 4;                                             // items per workgroup
    const int64_t n_launch = item_hi >= 0 ? (int64_t)(item_hi - item_lo) : pv.L.max_items;
    const unsigned blocks = hgt_item_grid((n_launch + IPW - 1) / IPW);
    if (lane_gather)
        k_edge_logits_kside<H, true><<<blocks, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, Q, K, table_bytes, img, logits, R, item_lo, item_hi, (int)pv.L.max_items);
    else
        k_edge_logits_kside<H, false><<<blocks, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, Q, K, table_bytes, img, logits, R, item_lo, item_hi, (int)pv.L.max_items);
}

// one head group of 32-column heads
static bool kside_layout(int32_t H, int32_t dk_pad) { return dk_pad == HGT_KSIDE_DK && (H == 2 || H == 4 || H == 8); }

}  // namespace

extern "C" int hgt_relation_kside_bytes(int32_t R, int32_t H, int32_t dk_pad, uint64_t* out) {
    if (!out || R <= 0 || H <= 0 || dk_pad <= 0) return HGT_ERR_INVALID_ARG;
    *out = kside_layout(H, dk_pad) ? (uint64_t)R * H * HGT_KSIDE_BLOCK_ELEMS * 2 + hgt_align_up((uint64_t)R * H * 4, 256) : 0;
    return HGT_OK;
}

extern "C" int hgt_relation_kside_pack(const float* att_t, int32_t R, int32_t H, int32_t dk_pad, void* att_kside, void* stream) {
    if (!att_t || !att_kside || R <= 0 || H <= 0 || dk_pad <= 0) return HGT_ERR_INVALID_ARG;
    if (!kside_layout(H, dk_pad)) return HGT_ERR_UNSUPPORTED;
    k_relation_kside_pack<<<(unsigned)(R * H), 256, 0, (hipStream_t)stream>>>(att_t, R * H, (unsigned short*)att_kside);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

// the work items [item_lo, item_hi) of the plan (a target block of the multi-GPU path), or all of them (0, -1)
__attribute__((visibility("hidden"))) int hgt_edge_logits_kside_items(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H,
                                                                      int32_t dk_pad, const float* Q, const float* K, const float* rte_k,
                                                                      const void* att_kside, float* logits, int item_lo, int item_hi, int lane_gather,
                                                                      void* stream) {
    if (!plan || !Q || !K || !att_kside || (E > 0 && !logits) || N < 0 || E < 0 || R <= 0 || H <= 0 || 64 % H != 0 || dk_pad <= 0)
        return HGT_ERR_INVALID_ARG;
    if (dk_pad % (64 / H) != 0) return HGT_ERR_INVALID_ARG;
    // covered: 32-column heads in one head group, no temporal rows, every Q / K row below 4 GiB from its base (32-bit lane offsets)
    if (!kside_layout(H, dk_pad) || rte_k || (uint64_t)N * (uint64_t)H * (uint64_t)dk_pad * 4u >= (1ull << 32)) return HGT_ERR_UNSUPPORTED;
    if (E == 0) return HGT_OK;
    const HgtPlanView pv = hgt_plan_view(plan, N, E, T, R);
    const unsigned short* img = (const unsigned short*)att_kside;
    const unsigned table_bytes = (unsigned)((uint64_t)N * H * dk_pad * 4u);      // (Q may have fewer rows: the plan's targets lie inside it)
    if (H == 2) launch_kside<2>(pv, Q, K, table_bytes, img, logits, R, item_lo, item_hi, lane_gather != 0, (hipStream_t)stream);
    else if (H == 4) launch_kside<4>(pv, Q, K, table_bytes, img, logits, R, item_lo, item_hi, lane_gather != 0, (hipStream_t)stream);
    else launch_kside<8>(pv, Q, K, table_bytes, img, logits, R, item_lo, item_hi, lane_gather != 0, (hipStream_t)stream);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_edge_logits_kside(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad,
                                     const float* Q, const float* K, const float* rte_k, const float* att_t, const void* att_kside,
                                     int32_t frag_f16, float* logits, void* stream) {
    (void)att_t;
    return hgt_edge_logits_kside_items(plan, N, E, T, R, H, dk_pad, Q, K, rte_k, att_kside, logits, 0, -1, frag_f16 & 8, stream);
}

// The index maps of hgt_kside_map.h enumerated on the host (no GPU): image_map[p] = {block, term, output, k} for every f16 element
// p of an image of n_blocks (relation, head) blocks; b_col[s][lane][j] = the K column a lane supplies as element j of k-step s;
// c_out[lane][reg] = the output a lane receives in accumulator register reg.  Any of the three may be NULL.
extern "C" int hgt_kside_image_map(int32_t n_blocks, int32_t* image_map, int32_t* b_col, int32_t* c_out) {
    if (n_blocks < 0) return HGT_ERR_INVALID_ARG;
    if (image_map)
        for (int64_t rh = 0; rh < n_blocks; ++rh)
            for (int s = 0; s < 2; ++s)
                for (int term = 0; term < 2; ++term)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            int32_t* o = image_map + 4 * hgt_kside_image_index(rh, s, term, lane, j);
                            o[0] = (int32_t)rh, o[1] = term, o[2] = hgt_kside_image_out(lane), o[3] = hgt_kside_image_k(s, lane, j);
                        }
    for (int lane = 0; lane < 64; ++lane) {
        if (b_col)
            for (int s = 0; s < 2; ++s)
                for (int j = 0; j < 8; ++j) b_col[(s * 64 + lane) * 8 + j] = hgt_kside_k_col(s, lane >> 5, j);
        if (c_out)
            for (int reg = 0; reg < 16; ++reg) c_out[lane * 16 + reg] = hgt_kside_c_out(lane >> 5, reg);
    }
    return HGT_OK;
}

// The gather maps of hgt_kside_map.h enumerated on the host (no GPU): dma_map[piece 4][lane 64] = {edge of the batch, chunk of the
// head line} a DMA lane fetches (its 16 bytes land at 1024 piece + 16 lane of the batch's 4 KB); read_map[i 4][lane 64] = {LDS byte
// offset, edge, chunk}: where read i of a lane goes and what it must find there.  Either may be NULL.
extern "C" int hgt_kside_gather_map(int32_t* dma_map, int32_t* read_map) {
    for (int lane = 0; lane < 64; ++lane)
        for (int p = 0; p < 4; ++p) {
            if (dma_map) {
                int32_t* o = dma_map + 2 * (p * 64 + lane);
                o[0] = hgt_kside_dma_edge(p, lane), o[1] = hgt_kside_dma_chunk(p, lane);
            }
            if (read_map) {
                int32_t* o = read_map + 3 * (p * 64 + lane);
                o[0] = hgt_kside_read_offset(lane, p), o[1] = lane & 31, o[2] = hgt_kside_read_chunk(lane, p);
            }
        }
    return HGT_OK;
}
