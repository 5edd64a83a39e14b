// Matcher retrieval (gfx950): the k best candidates of every query, and the exact rank of one candidate per query, over ALL candidates
// without the [N, Q] score matrix.
//
//   hgt_matcher_topk   values / indices [Q, k] of s(c, q) = (tx_c . ty_q) * scale, best first
//   hgt_matcher_rank   rank[q] = #{ c : c comes before index[q] in the order of query q }
//
// Score.  One v_mfma_f32_32x32x2_f32 chain per pair, the same wherever a pair is computed (tile_scores below): the candidate rows are
// operand A, the query rows operand B, and the d columns are taken 32 at a time -- lane half h = lane >> 5 owns columns
// kb + 16 h .. kb + 16 h + 15, and step m = 0 .. 15 of a 32-column block multiplies column kb + m (half 0), then kb + 16 + m (half 1),
// into the accumulator: a k-ordered fp32 fma chain from +0 whose order depends on d alone.  Columns past d are zeros (a group of four
// steps whose both halves lie past d is skipped).  The finished sum is multiplied by `scale` once.  So the bits of s(c, q) are a function
// of row c of tx, row q of ty, d and scale -- not of the tile a pair falls in, the chunking, N or Q -- and the top-k pass, the rank
// pass and the target's own score (the diagonal of one more tile on the gathered target rows) see the same bits.
//
// Order.  A pair is ranked by a 64-bit key: upper word = a monotone image of the float (-0 -> +0, every NaN -> the positive quiet NaN,
// which stands above +inf), lower word = ~position.  Keys are distinct, larger = earlier, 0 = no entry.  Selection is integer only.
//
// Pass.  A workgroup (4 wavefronts) takes one block of 32 or 64 queries and one chunk of candidate rows.  Per round every wavefront
// forms the scores of 32 candidates x the query block (1 or 2 accumulators of 16 registers), straight from global memory: a lane loads
// 64 consecutive bytes of its candidate row and of its query rows per 32-column block (the query block stays in L1 / L2; fp32 MFMA is
// slow enough that 12 16-byte loads per 32 instructions stay under half the L1 rate).  top-k: a key above the query's threshold (the
// k-th key kept so far, 0 at first) is appended to the query's LDS list (an integer LDS counter hands out slots: the slot order is
// arbitrary, the set of keys is not); a full list makes the whole workgroup sort every list (bitonic, descending), keep k, raise the
// thresholds and offer the refused keys again.  A key is only ever dropped below k larger ones, so the k kept are the k best of the
// chunk whatever the order of arrival.  The chunk's lists go to the workspace; k_merge (a workgroup per query) runs the same
// append / sort over the chunks' lists and decodes keys into values and indices.  rank: the same stream, counting keys above the
// target's; per-chunk integer counts go to the workspace and k_rank_sum adds them.
//
// LDS (static): lists of CAP = max(64, 2 * pow2(k)) keys per query: 32 KB (k <= 32, 64 queries), 64 KB (k <= 64, 64 queries; k <= 128,
// 32 queries), plus a threshold and a counter per query.  Registers: 32 accumulators + 2 x 48 fragment registers (the next block's
// loads are issued before this block's MFMAs).
#include <limits.h>
#include <math.h>

#include "hgt_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int MT_BLOCK = 256;
constexpr int MT_WAVES = MT_BLOCK / 64;
constexpr int MT_TILE = 32;                          // candidates of one wavefront's tile
constexpr int MT_ROUND = MT_WAVES * MT_TILE;         // candidates of one round of a workgroup: the unit chunk_rows is rounded to
constexpr int MT_MERGE_CAP = 512;                    // keys of k_merge's list
constexpr int64_t MT_MIN_CHUNK = 2048;               // the shortest chunk the library chooses itself
constexpr int64_t MT_TARGET_GROUPS = 1024;           // workgroups the library aims at (256 CUs x a few)
static_assert(MT_MERGE_CAP >= 2 * HGT_TOPK_MAX_K, "k_merge keeps k keys and takes at least k more before it sorts");

struct Plan {
    int nq, qb, cap, n_qb;
    int64_t rows, n_chunks;
};

inline int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p *= 2;
    return p;
}

// the launch geometry: a function of the four numbers the workspace question is asked with
inline Plan plan_for(int64_t n_cand, int64_t n_query, int k, int64_t chunk_rows) {
    Plan P;
    P.nq = (n_query > 32 && k <= 64) ? 2 : 1;
    P.qb = 32 * P.nq;
    const int c = 2 * pow2_at_least(k);
    P.cap = c < 64 ? 64 : c;
    P.n_qb = (int)((n_query + P.qb - 1) / P.qb);
    if (chunk_rows > 0) {
        P.rows = (chunk_rows + MT_ROUND - 1) / MT_ROUND * MT_ROUND;
    } else {
        const int64_t want = MT_TARGET_GROUPS / (P.n_qb > 0 ? P.n_qb : 1) > 0 ? MT_TARGET_GROUPS / (P.n_qb > 0 ? P.n_qb : 1) : 1;
        int64_t r = (n_cand + want - 1) / want;
        if (r < MT_MIN_CHUNK) r = MT_MIN_CHUNK;
        P.rows = (r + MT_ROUND - 1) / MT_ROUND * MT_ROUND;
    }
    P.n_chunks = (n_cand + P.rows - 1) / P.rows;
    return P;
}

__device__ inline u64 key_of(float s, int pos) {
    uint32_t u = __float_as_uint(s);
    if (s != s) u = 0x7FC00000u;
    if (u == 0x80000000u) u = 0u;
    const uint32_t m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)m << 32) | (uint32_t)~(uint32_t)pos;
}

__device__ inline float value_of(u64 key) {
    const uint32_t m = (uint32_t)(key >> 32);
    return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}

__device__ inline int pos_of(u64 key) { return (int)~(uint32_t)key; }

__device__ inline float4 load4(const float* p, bool vec) {
    if (vec) return *(const float4*)p;
    return make_float4(p[0], p[1], p[2], p[3]);
}

// row of the 32 x 32 result a lane holds in accumulator register r
__device__ inline int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

template <int NQ>
struct Frag {
    float4 a[4];
    float4 b[NQ][4];
};

template <int NQ>
__device__ inline void load_frag(Frag<NQ>& f, const float* arow, const float* const (&brow)[NQ], int k0, int d, bool vec) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int kk = k0 + 4 * t;
        const bool in = kk < d;
        f.a[t] = (arow && in) ? load4(arow + kk, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int n = 0; n < NQ; ++n) f.b[n][t] = (brow[n] && in) ? load4(brow[n] + kk, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// THE score chain: acc[n] (row = candidate of the tile, column = query lane & 31 of half-block n) = tx rows . ty rows, unscaled.
// arow / brow[n]: this lane's candidate row (row lane & 31 of the tile) and query rows, NULL = a row of zeros.
template <int NQ>
__device__ inline void tile_scores(const float* arow, const float* const (&brow)[NQ], int d, bool vec, f32x16 (&acc)[NQ]) {
    const int h16 = 16 * ((threadIdx.x & 63) >> 5);
#pragma unroll
    for (int n = 0; n < NQ; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    Frag<NQ> f;
    load_frag<NQ>(f, arow, brow, h16, d, vec);
    for (int kb = 0; kb < d; kb += 32) {
        Frag<NQ> g;
        if (kb + 32 < d) load_frag<NQ>(g, arow, brow, kb + 32 + h16, d, vec);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (kb + 4 * t < d) {                                     // (uniform: half 0's columns of this group exist)
#pragma unroll
                for (int n = 0; n < NQ; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[t].x, f.b[n][t].x, acc[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NQ; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[t].y, f.b[n][t].y, acc[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NQ; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[t].z, f.b[n][t].z, acc[n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < NQ; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[t].w, f.b[n][t].w, acc[n], 0, 0, 0);
            }
        }
        if (kb + 32 < d) f = g;
    }
}

struct MatchArgs {
    const float* tx;
    const float* ty;
    int64_t ld_x, ld_y;
    int32_t n_cand, n_query, d, k;
    float scale;
    int32_t vec;             // every row of tx and ty is 16-byte aligned
    int32_t n_qb;
    int64_t rows, n_chunks;
    u64* part;               // top-k: [n_chunks][n_query][k] keys
    int32_t* counts;         // rank: [n_chunks][n_query]
    const int64_t* index;
};

template <int NQ>
__device__ inline void query_rows(const MatchArgs& A, int q0, const float* (&brow)[NQ]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const int q = q0 + 32 * n + (lane & 31);
        brow[n] = q < A.n_query ? A.ty + (int64_t)q * A.ld_y : nullptr;
    }
}

// ------------------------------------------------------------------------------------------------ the lists
// Every list of `cap` keys (a power of two) sorted descending by the whole workgroup; ends with a barrier.
__device__ inline void sort_lists(u64* buf, int n_lists, int cap) {
    const int half = cap >> 1, total = n_lists * half;
    for (int size = 2; size <= cap; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < total; t += blockDim.x) {
                const int list = t / half, p = t - list * half;
                const int i = (p / stride) * 2 * stride + (p % stride), j = i + stride;
                u64* L = buf + list * cap;
                const u64 a = L[i], b = L[j];
                const bool desc = (i & size) == 0;
                if ((a < b) == desc && a != b) {
                    L[i] = b;
                    L[j] = a;
                }
            }
            __syncthreads();
        }
    }
}

// Keep the k best of every list, raise the thresholds, clear the overflow flag.  Called by the whole workgroup after a barrier.
__device__ inline void compact_lists(u64* buf, int* cnt, u64* thr, int* flag, int n_lists, int cap, int k) {
    for (int t = threadIdx.x; t < n_lists * cap; t += blockDim.x) {
        const int list = t / cap, s = t - list * cap;
        if (s >= cnt[list]) buf[t] = 0ull;                    // (a count beyond cap: every slot is taken)
    }
    __syncthreads();
    sort_lists(buf, n_lists, cap);
    for (int q = threadIdx.x; q < n_lists; q += blockDim.x) {
        int c = cnt[q] < cap ? cnt[q] : cap;
        c = c < k ? c : k;
        cnt[q] = c;
        thr[q] = c == k ? buf[q * cap + k - 1] : 0ull;
    }
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
}

// One offer of `key` (0 = nothing) to list q: true = settled (kept or below the threshold), false = the list was full.
__device__ inline bool offer(u64 key, int q, u64* buf, int* cnt, const volatile u64* thr, int cap) {
    if (key <= thr[q]) return true;
    const int slot = atomicAdd(&cnt[q], 1);
    if (slot >= cap) return false;
    buf[q * cap + slot] = key;
    return true;
}

// ------------------------------------------------------------------------------------------------ top-k over one chunk
template <int NQ, int CAP>
__global__ void __launch_bounds__(MT_BLOCK) k_topk_chunk(MatchArgs A) {
    constexpr int QB = 32 * NQ;
    constexpr int cap = CAP;
    __shared__ u64 buf[QB * CAP];
    __shared__ u64 thr[QB];
    __shared__ int cnt[QB];
    __shared__ int flag[1];
    const int k = A.k;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qb = blockIdx.x % A.n_qb;
    const int64_t chunk = blockIdx.x / A.n_qb;
    const int q0 = qb * QB;
    const int64_t c0 = chunk * A.rows;
    const int64_t c1 = c0 + A.rows < A.n_cand ? c0 + A.rows : A.n_cand;
    for (int q = threadIdx.x; q < QB; q += MT_BLOCK) {
        thr[q] = 0ull;
        cnt[q] = 0;
    }
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    const float* brow[NQ];
    query_rows<NQ>(A, q0, brow);
    for (int64_t base = c0; base < c1; base += MT_ROUND) {          // (uniform over the workgroup)
        const int64_t r0 = base + wave * MT_TILE;
        const int64_t my = r0 + (lane & 31);
        const float* arow = my < c1 ? A.tx + my * A.ld_x : nullptr;
        f32x16 acc[NQ];
        tile_scores<NQ>(arow, brow, A.d, A.vec != 0, acc);
        uint32_t pend[NQ];
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            pend[n] = 0;
            const int ql = 32 * n + (lane & 31);
            if (q0 + ql < A.n_query) {
                const u64 t = ((const volatile u64*)thr)[ql];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = r0 + acc_row(r, lane);
                    if (row < c1 && key_of(acc[n][r] * A.scale, (int)row) > t) pend[n] |= 1u << r;
                }
            }
        }
        for (;;) {
            bool refused = false;
#pragma unroll
            for (int n = 0; n < NQ; ++n) {
                const int ql = 32 * n + (lane & 31);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (pend[n] & (1u << r)) {
                        const int row = (int)(r0 + acc_row(r, lane));
                        if (offer(key_of(acc[n][r] * A.scale, row), ql, buf, cnt, thr, cap)) pend[n] &= ~(1u << r);
                        else refused = true;
                    }
                }
            }
            if (refused) *(volatile int*)flag = 1;
            __syncthreads();
            const int full = *(volatile int*)flag;
            __syncthreads();
            if (!full) break;
            compact_lists(buf, cnt, thr, flag, QB, cap, k);
        }
    }
    __syncthreads();
    compact_lists(buf, cnt, thr, flag, QB, cap, k);
    for (int t = threadIdx.x; t < QB * k; t += MT_BLOCK) {
        const int ql = t / k, s = t - ql * k;
        if (q0 + ql < A.n_query) A.part[(chunk * A.n_query + q0 + ql) * k + s] = s < cnt[ql] ? buf[ql * cap + s] : 0ull;
    }
}

// ------------------------------------------------------------------------------------------------ the chunks' lists of one query
__global__ void __launch_bounds__(MT_BLOCK) k_merge(const u64* part, int64_t n_chunks, int32_t n_query, int32_t k, float* values,
                                                    int64_t* indices) {
    __shared__ u64 buf[MT_MERGE_CAP];
    __shared__ u64 thr[1];
    __shared__ int cnt[1];
    __shared__ int flag[1];
    const int q = blockIdx.x;
    if (threadIdx.x == 0) {
        thr[0] = 0ull;
        cnt[0] = 0;
        flag[0] = 0;
    }
    __syncthreads();
    const int64_t total = n_chunks * k;
    for (int64_t base = 0; base < total; base += MT_BLOCK) {
        const int64_t e = base + threadIdx.x;
        u64 key = 0ull;
        if (e < total) {
            const int64_t c = e / k;
            key = part[(c * n_query + q) * k + (e - c * k)];
        }
        bool pending = key != 0ull;
        for (;;) {
            if (pending) {
                if (offer(key, 0, buf, cnt, thr, MT_MERGE_CAP)) pending = false;
                else *(volatile int*)flag = 1;
            }
            __syncthreads();
            const int full = *(volatile int*)flag;
            __syncthreads();
            if (!full) break;
            compact_lists(buf, cnt, thr, flag, 1, MT_MERGE_CAP, k);
        }
    }
    __syncthreads();
    compact_lists(buf, cnt, thr, flag, 1, MT_MERGE_CAP, k);
    for (int s = threadIdx.x; s < k; s += MT_BLOCK) {
        const bool in = s < cnt[0];
        values[(int64_t)q * k + s] = in ? value_of(buf[s]) : -INFINITY;
        indices[(int64_t)q * k + s] = in ? (int64_t)pos_of(buf[s]) : -1ll;
    }
}

// ------------------------------------------------------------------------------------------------ ranks over one chunk
template <int NQ>
__global__ void __launch_bounds__(MT_BLOCK) k_rank_chunk(MatchArgs A) {
    constexpr int QB = 32 * NQ;
    __shared__ u64 tkey[QB];
    __shared__ int total[QB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qb = blockIdx.x % A.n_qb;
    const int64_t chunk = blockIdx.x / A.n_qb;
    const int q0 = qb * QB;
    const int64_t c0 = chunk * A.rows;
    const int64_t c1 = c0 + A.rows < A.n_cand ? c0 + A.rows : A.n_cand;
    const float* brow[NQ];
    query_rows<NQ>(A, q0, brow);
    for (int q = threadIdx.x; q < QB; q += MT_BLOCK) total[q] = 0;
    // the targets' own scores: tile n of wavefront n pairs target row i with query i, the diagonal of the same chain
    if (wave < NQ) {
        const int q = q0 + 32 * wave + (lane & 31);
        int64_t tgt = -1;
        if (q < A.n_query) {
            tgt = A.index[q];
            if (tgt < 0 || tgt >= A.n_cand) tgt = -1;
        }
        const float* arow = tgt >= 0 ? A.tx + tgt * A.ld_x : nullptr;
        const float* b1[1] = {wave == 0 ? brow[0] : brow[NQ - 1]};
        f32x16 acc[1];
        tile_scores<1>(arow, b1, A.d, A.vec != 0, acc);
        const int j = lane & 31;
        if (((j >> 2) & 1) == (lane >> 5)) {                  // the lane half that holds row j of column j
            const int want = (j & 3) + 4 * (j >> 3);
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (r == want) s = acc[0][r];
            tkey[32 * wave + j] = tgt >= 0 ? key_of(s * A.scale, (int)tgt) : 0ull;          // 0 = no target
        }
    }
    __syncthreads();
    u64 mine[NQ];
    int count[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        mine[n] = tkey[32 * n + (lane & 31)];
        count[n] = 0;
    }
    for (int64_t r0 = c0 + wave * MT_TILE; r0 < c1; r0 += MT_ROUND) {
        const int64_t my = r0 + (lane & 31);
        const float* arow = my < c1 ? A.tx + my * A.ld_x : nullptr;
        f32x16 acc[NQ];
        tile_scores<NQ>(arow, brow, A.d, A.vec != 0, acc);
#pragma unroll
        for (int n = 0; n < NQ; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = r0 + acc_row(r, lane);
                count[n] += (row < c1 && key_of(acc[n][r] * A.scale, (int)row) > mine[n]) ? 1 : 0;
            }
    }
#pragma unroll
    for (int n = 0; n < NQ; ++n)
        if (count[n]) atomicAdd(&total[32 * n + (lane & 31)], count[n]);          // integer adds: the sum has no order
    __syncthreads();
    for (int q = threadIdx.x; q < QB; q += MT_BLOCK)
        if (q0 + q < A.n_query) A.counts[chunk * A.n_query + q0 + q] = total[q];
}

__global__ void __launch_bounds__(MT_BLOCK) k_rank_sum(const int32_t* counts, int64_t n_chunks, int32_t n_query, int32_t n_cand,
                                                       const int64_t* index, int64_t* rank) {
    const int q = blockIdx.x * MT_BLOCK + threadIdx.x;
    if (q >= n_query) return;
    const int64_t t = index[q];
    if (t < 0 || t >= n_cand) {
        rank[q] = -1;
        return;
    }
    int64_t sum = 0;
    for (int64_t c = 0; c < n_chunks; ++c) sum += counts[c * n_query + q];
    rank[q] = sum;
}

// ------------------------------------------------------------------------------------------------ host
constexpr int64_t MT_LIMIT = (1ll << 31) - 1;

int sizes_ok(int64_t n_cand, int64_t n_query, int32_t k, int64_t chunk_rows) {
    if (n_cand < 0 || n_query < 0 || k < 1 || chunk_rows < 0) return HGT_ERR_INVALID_ARG;
    if (k > HGT_TOPK_MAX_K || n_query >= MT_LIMIT) return HGT_ERR_UNSUPPORTED;
    if (n_cand >= MT_LIMIT) return HGT_ERR_TOO_LARGE;
    return HGT_OK;
}

// bytes of the per-chunk lists (8 k per chunk and query; the rank pass asks with k = 1 and uses 4); too many workgroups: TOO_LARGE
int bytes_for(const Plan& P, int64_t n_query, int32_t k, uint64_t* out) {
    const unsigned __int128 groups = (unsigned __int128)P.n_chunks * (unsigned)P.n_qb;
    const unsigned __int128 b = (unsigned __int128)P.n_chunks * (uint64_t)n_query * (uint64_t)k * 8u;
    if (groups >= (unsigned __int128)MT_LIMIT || b > ((unsigned __int128)1 << 62)) return HGT_ERR_TOO_LARGE;
    *out = hgt_align_up((uint64_t)b, 256) + 256;
    return HGT_OK;
}

int args_ok(const float* tx, int64_t ld_x, int64_t n_cand, const float* ty, int64_t ld_y, int64_t n_query, int32_t d, float scale, int32_t k,
            int64_t chunk_rows) {
    if (d < 0 || !(scale == scale) || isinf(scale)) return HGT_ERR_INVALID_ARG;
    const int rc = sizes_ok(n_cand, n_query, k, chunk_rows);
    if (rc == HGT_ERR_INVALID_ARG) return rc;
    if (ld_x < d || ld_y < d) return HGT_ERR_INVALID_ARG;
    if ((n_cand > 0 && !tx) || (n_query > 0 && !ty)) return HGT_ERR_INVALID_ARG;
    if (rc != HGT_OK) return rc;
    if (d < 4 || d % 4 != 0 || d > 1024) return HGT_ERR_UNSUPPORTED;
    return HGT_OK;
}

MatchArgs make_args(const Plan& P, const float* tx, int64_t ld_x, int64_t n_cand, const float* ty, int64_t ld_y, int64_t n_query, int32_t d,
                    float scale, int32_t k) {
    MatchArgs A = {};
    A.tx = tx; A.ty = ty; A.ld_x = ld_x; A.ld_y = ld_y;
    A.n_cand = (int32_t)n_cand; A.n_query = (int32_t)n_query; A.d = d; A.k = k; A.scale = scale;
    A.vec = (((uintptr_t)tx | (uintptr_t)ty) % 16 == 0 && ld_x % 4 == 0 && ld_y % 4 == 0) ? 1 : 0;
    A.n_qb = P.n_qb; A.rows = P.rows; A.n_chunks = P.n_chunks;
    return A;
}

}  // namespace

extern "C" int hgt_matcher_topk_bytes(int64_t n_cand, int64_t n_query, int32_t k, int64_t chunk_rows, uint64_t* bytes_host) {
    if (!bytes_host) return HGT_ERR_INVALID_ARG;
    const int rc = sizes_ok(n_cand, n_query, k, chunk_rows);
    if (rc != HGT_OK) return rc;
    return bytes_for(plan_for(n_cand, n_query, k, chunk_rows), n_query, k, bytes_host);
}

extern "C" int hgt_matcher_topk(const float* tx, int64_t ld_x, int64_t n_cand, const float* ty, int64_t ld_y, int64_t n_query, int32_t d,
                                float scale, int32_t k, int64_t chunk_rows, float* values_out, int64_t* indices_out, void* ws,
                                uint64_t ws_bytes, void* stream) {
    const int rc = args_ok(tx, ld_x, n_cand, ty, ld_y, n_query, d, scale, k, chunk_rows);
    if (rc != HGT_OK) return rc;
    if (n_query == 0) return HGT_OK;
    if (!values_out || !indices_out) return HGT_ERR_INVALID_ARG;
    const Plan P = plan_for(n_cand, n_query, k, chunk_rows);
    uint64_t need = 0;
    const int rb = bytes_for(P, n_query, k, &need);
    if (rb != HGT_OK) return rb;
    if (!ws || ws_bytes < need) return HGT_ERR_WORKSPACE;
    MatchArgs A = make_args(P, tx, ld_x, n_cand, ty, ld_y, n_query, d, scale, k);
    A.part = (u64*)ws;
    if (P.n_chunks > 0) {
        const unsigned grid = (unsigned)(P.n_chunks * P.n_qb);
        const hipStream_t st = (hipStream_t)stream;
        if (P.cap == 64 && P.nq == 2) k_topk_chunk<2, 64><<<grid, MT_BLOCK, 0, st>>>(A);
        else if (P.cap == 64) k_topk_chunk<1, 64><<<grid, MT_BLOCK, 0, st>>>(A);
        else if (P.cap == 128 && P.nq == 2) k_topk_chunk<2, 128><<<grid, MT_BLOCK, 0, st>>>(A);
        else if (P.cap == 128) k_topk_chunk<1, 128><<<grid, MT_BLOCK, 0, st>>>(A);
        else k_topk_chunk<1, 256><<<grid, MT_BLOCK, 0, st>>>(A);
        HGT_CHECK_LAUNCH();
    }
    k_merge<<<(unsigned)n_query, MT_BLOCK, 0, (hipStream_t)stream>>>(A.part, P.n_chunks, (int32_t)n_query, k, values_out, indices_out);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_matcher_rank(const float* tx, int64_t ld_x, int64_t n_cand, const float* ty, int64_t ld_y, int64_t n_query, int32_t d,
                                float scale, int64_t chunk_rows, const int64_t* index, int64_t* rank_out, void* ws, uint64_t ws_bytes,
                                void* stream) {
    const int rc = args_ok(tx, ld_x, n_cand, ty, ld_y, n_query, d, scale, 1, chunk_rows);
    if (rc != HGT_OK) return rc;
    if (n_query == 0) return HGT_OK;
    if (!index || !rank_out) return HGT_ERR_INVALID_ARG;
    const Plan P = plan_for(n_cand, n_query, 1, chunk_rows);
    uint64_t need = 0;
    const int rb = bytes_for(P, n_query, 1, &need);
    if (rb != HGT_OK) return rb;
    if (!ws || ws_bytes < need) return HGT_ERR_WORKSPACE;
    MatchArgs A = make_args(P, tx, ld_x, n_cand, ty, ld_y, n_query, d, scale, 1);
    A.counts = (int32_t*)ws;
    A.index = index;
    if (P.n_chunks > 0) {
        const unsigned grid = (unsigned)(P.n_chunks * P.n_qb);
        if (P.nq == 2) k_rank_chunk<2><<<grid, MT_BLOCK, 0, (hipStream_t)stream>>>(A);
        else k_rank_chunk<1><<<grid, MT_BLOCK, 0, (hipStream_t)stream>>>(A);
        HGT_CHECK_LAUNCH();
    }
    k_rank_sum<<<(unsigned)((n_query + MT_BLOCK - 1) / MT_BLOCK), MT_BLOCK, 0, (hipStream_t)stream>>>(A.counts, P.n_chunks, (int32_t)n_query,
                                                                                                     (int32_t)n_cand, index, rank_out);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}
