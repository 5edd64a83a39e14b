// Exact L-hop neighbourhood of a seed set from the resident graph: a frontier walk over the in-edge CSRs (row = target, entries =
// sources) whose result stands in the seed trim's hop-major order, so every layer runs as the rectangular layer on a prefix.
// include/hgt_hip.h states the contract; the numpy definition is pyhgt_amd.neighbourhood.np_neighbourhood.
//
//   state      one resident int32 mark per node (per type): -1 idle, HGT_NB_CLAIMED between a claim and its number, then the node's
//              new row.  Nothing else is proportional to the graph: every grid, loop and scratch array below is sized by a level, by
//              its CSR entries, or by the seeds.  hgt_nb_reset walks a level's own key list to put the marks back.
//   levels     level 0 = the distinct seeds; level h + 1 = the sources of the kept entries of level h's rows that had no mark.  A
//              claim is an integer compare-and-swap -1 -> CLAIMED (every writer writes the same value: the SET does not depend on
//              arrival order); the winner writes its key (type << 32 | id) into a candidate list at the place of the ENTRY that
//              claimed it (the list has one slot per CSR entry of the level and starts as all-ones keys: no counter, no shared
//              address).  The ORDER never comes from that list: it is radix-sorted (rocPRIM; the all-ones keys go last), and a
//              node's number is level offset + rank.
//   edges      an item is (level-h row, triple whose target type is the row's type), triple-major: the view's order.  A row of more
//              than HGT_NB_CHUNK entries is split into chunks; one wavefront takes one chunk, its lanes striding the entries.  Count
//              pass (kept entries per chunk, and the claims) -> one single-workgroup scan -> fill pass (after level h + 1 has its
//              numbers: it reads the sources' new rows from the marks), a kept entry's position = the scan's value for its chunk + the
//              kept entries of the wavefront's earlier steps + its rank in a ballot.  The self loops of the bucket follow.
//   predicate  the whole-graph view's, from the one statement both call (hgt_graph_rule.h: entry_kept, entry_time_diff); a time
//              difference outside [0, 240) is written as it is and sets HGT_NB_BAD_TIME.
// Integers only, vector stores only; the atomics are the claim, the level totals and the OR into the flag word -- none of them
// decides a position.  Nothing here synchronises: the caller reads the head once per level.
#include <rocprim/device/device_radix_sort.hpp>

#include "hgt_graph_rule.h"

namespace {

constexpr int BS = 256;
constexpr int CHUNK = HGT_NB_CHUNK;
constexpr int WAVE_ROWS = HGT_NB_WAVE_ROWS;          // rows whose entry and chunk totals one wavefront sums before its one atomic add
static_assert(WAVE_ROWS == 64 && BS % WAVE_ROWS == 0, "a wavefront of gfx950");
constexpr int SCAN_BS = 1024;
constexpr int64_t LIMIT = (1ll << 31) - 1;
constexpr int32_t CLAIMED = HGT_NB_CLAIMED;
constexpr uint64_t PAD_KEY = ~0ull;
constexpr int MAX_T = HGT_SAMPLER_MAX_TYPES, MAX_M = HGT_SAMPLER_MAX_TRIPLES;

typedef unsigned long long u64;

// head words (int64): include/hgt_hip.h
enum { H_N = HGT_NB_HEAD_N, H_DEG = HGT_NB_HEAD_DEG, H_CHUNKS = HGT_NB_HEAD_CHUNKS, H_KEPT = HGT_NB_HEAD_KEPT, H_FLAGS = HGT_NB_HEAD_FLAGS,
       H_BEGIN = HGT_NB_HEAD_TYPE_BEGIN, H_END = HGT_NB_HEAD_TYPE_END };

static inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

__device__ __forceinline__ u64 make_key(int32_t type, int32_t id) { return ((u64)(uint32_t)type << 32) | (uint32_t)id; }

// the items of one level, triple-major: item j of triple m is the level row row0[m] + (j - base[m])
struct ItemTab {
    int32_t base[MAX_M + 1];
    int32_t row0[MAX_M];
    int32_t M, n_items;
};

__global__ void k_nb_head_set(int64_t* head, int mode) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (mode == 0) {                                    // a new call
        for (int i = 0; i < HGT_NB_HEAD_WORDS; ++i) head[i] = 0;
    } else if (mode == 1) {                             // before a level's claims
        head[H_N] = 0; head[H_KEPT] = 0;
    } else {                                            // before a level gets its numbers
        head[H_N] = 0; head[H_DEG] = 0; head[H_CHUNKS] = 0;
        for (int i = H_BEGIN; i < HGT_NB_HEAD_WORDS; ++i) head[i] = 0;
    }
}

__global__ __launch_bounds__(BS) void k_nb_seeds(const hgt_nb_type* __restrict__ types, int32_t T, const int32_t* __restrict__ seed_type,
                                                 const int64_t* __restrict__ seed_id, int64_t S, uint64_t* __restrict__ cand,
                                                 int64_t* __restrict__ head) {
    const int64_t s = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (s >= S) return;
    const int32_t t = seed_type[s];
    const int64_t id = seed_id[s];
    if (t < 0 || t >= T || id < 0 || id >= types[t].n_nodes) {
        atomicOr((u64*)&head[H_FLAGS], (u64)HGT_NB_BAD_SEED);
        return;
    }
    if (atomicCAS(&types[t].mark[id], -1, CLAIMED) == -1) cand[s] = make_key(t, (int32_t)id);    // (the other slots stay all-ones)
}

// the keys of the sorted list that are not all-ones are the level: they get their numbers, and their count goes to head[H_N] (zeroed
// before); with `expand` the level's CSR entries and chunks are summed
__global__ __launch_bounds__(BS) void k_nb_number(const hgt_nb_type* __restrict__ types, const hgt_nb_triple* __restrict__ tri, int32_t M,
                                                  const uint64_t* __restrict__ keys, int64_t cap, int64_t row_base, int32_t expand,
                                                  int64_t* __restrict__ order, int64_t* __restrict__ node_type, int64_t* __restrict__ row_id,
                                                  int64_t* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    u64 deg = 0, chunks = 0;
    const uint64_t key = i < cap ? keys[i] : PAD_KEY;
    if (key != PAD_KEY) {
        const int32_t t = (int32_t)(key >> 32), id = (int32_t)(uint32_t)key;
        types[t].mark[id] = (int32_t)(row_base + i);
        order[i] = types[t].row_off + id;
        node_type[i] = t;
        row_id[i] = id;
        if (i == 0 || (int32_t)(keys[i - 1] >> 32) != t) head[H_BEGIN + t] = i;
        const uint64_t next = i + 1 < cap ? keys[i + 1] : PAD_KEY;
        if ((int32_t)(next >> 32) != t) head[H_END + t] = i + 1;          // (an all-ones key has no type)
        if (next == PAD_KEY) head[H_N] = i + 1;
        if (expand)
            for (int m = 0; m < M; ++m)
                if (tri[m].tgt_type == t) {
                    const int32_t d = tri[m].indptr[id + 1] - tri[m].indptr[id];
                    deg += (u64)d;
                    chunks += (u64)((d + CHUNK - 1) / CHUNK);
                }
    }
    if (!expand) return;
    for (int s = WAVE_ROWS / 2; s >= 1; s >>= 1) {
        deg += __shfl_xor(deg, s);
        chunks += __shfl_xor(chunks, s);
    }
    if ((threadIdx.x & (WAVE_ROWS - 1)) == 0 && (deg | chunks)) {
        atomicAdd((u64*)&head[H_DEG], deg);
        atomicAdd((u64*)&head[H_CHUNKS], chunks);
    }
}

__device__ __forceinline__ int item_triple(const ItemTab& it, int32_t j) {
    int m = 0;
    while (m + 1 < it.M && it.base[m + 1] <= j) ++m;
    return m;
}

__global__ __launch_bounds__(BS) void k_nb_items(const hgt_nb_triple* __restrict__ tri, ItemTab it, const uint64_t* __restrict__ keys,
                                                 int32_t* __restrict__ item_chunks, int32_t* __restrict__ item_entries) {
    const int32_t j = blockIdx.x * BS + threadIdx.x;
    if (j >= it.n_items) return;
    const int m = item_triple(it, j);
    const int32_t id = (int32_t)(uint32_t)keys[it.row0[m] + (j - it.base[m])];
    const int32_t d = tri[m].indptr[id + 1] - tri[m].indptr[id];
    item_chunks[j] = (d + CHUNK - 1) / CHUNK;
    item_entries[j] = d;
}

// exclusive scan of a[0, n] by ONE workgroup: a[n] becomes the total, which also goes to *total_out (may be NULL)
__global__ __launch_bounds__(SCAN_BS) void k_nb_scan(int32_t* __restrict__ a, int64_t n, int64_t* total_out) {
    __shared__ int32_t wsum[SCAN_BS / 64];
    __shared__ int32_t carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { carry = 0; a[n] = 0; }
    __syncthreads();
    for (int64_t b0 = 0; b0 <= n; b0 += SCAN_BS) {
        const int64_t i = b0 + threadIdx.x;
        const int32_t v = i <= n ? a[i] : 0;
        int32_t x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int w = 0; w < SCAN_BS / 64; ++w) {
            const int32_t sw = wsum[w];
            if (w < wave) before += sw;
            total += sw;
        }
        const int32_t c = carry;
        if (i <= n) a[i] = c + before + x - v;
        __syncthreads();
        if (threadIdx.x == 0) carry = c + total;
        __syncthreads();
    }
    if (threadIdx.x == 0 && total_out) *total_out = carry;
}

struct WalkArgs {
    const hgt_nb_type* types; const hgt_nb_triple* tri;
    const uint64_t* keys;                              // the level's sorted keys
    const int32_t* item_off;                           // [n_items + 1]: chunks in front of an item
    const int32_t* entry_off;                          // [n_items + 1]: CSR entries in front of an item (count pass)
    int32_t* chunk_cnt;                                // [n_chunks + 1]: kept entries per chunk; scanned between the two passes
    int64_t n_chunks;
    int32_t has_max_time, max_time;
    int64_t* head;
    // count pass
    uint64_t* cand; int64_t cand_cap;
    // fill pass
    int64_t row_base; int64_t* src; int64_t* dst; int64_t* etype; int64_t* etime; int64_t edge_cap;
};

// One wavefront, one chunk of one row.  FILL = false: counts the kept entries and claims their sources.  FILL = true: writes them.
template <bool FILL>
__global__ __launch_bounds__(BS) void k_nb_walk(WalkArgs a, ItemTab it) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6);
    if (c >= a.n_chunks) return;                                       // (a whole wavefront)
    int32_t lo = 0, hi = it.n_items - 1;                               // the last item j with item_off[j] <= c
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (a.item_off[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const int32_t j = lo;
    const int m = item_triple(it, j);
    const hgt_nb_triple tr = a.tri[m];
    const int32_t lrow = it.row0[m] + (j - it.base[m]);                // the row's place in its level
    const int32_t row = (int32_t)(uint32_t)a.keys[lrow];
    const int64_t p0 = (int64_t)tr.indptr[row] + (c - a.item_off[j]) * CHUNK;
    const int64_t row_end = tr.indptr[row + 1];
    const int64_t p1 = p0 + CHUNK < row_end ? p0 + CHUNK : row_end;
    int32_t* src_mark = a.types[tr.src_type].mark;
    const int32_t base = FILL ? a.chunk_cnt[c] : 0;
    int32_t kept = 0;
    bool bad = false;
    for (int64_t q = p0; q < p1; q += 64) {
        const int64_t p = q + lane;
        bool k = false;
        int32_t sl = 0;
        if (p < p1) {
            sl = tr.src[p];
            k = entry_kept(tr, row, p, sl, a.has_max_time, a.max_time);
        }
        const unsigned long long mask = __ballot(k);
        if (!FILL) {
            // (a plain look first: most sources of a level are claimed already -- a field of study by every paper in it -- and a
            //  compare-and-swap per entry on those few addresses serialises the pass; a stale -1 only costs the swap it would have made)
            const bool won = k && __atomic_load_n(&src_mark[sl], __ATOMIC_RELAXED) == -1 && atomicCAS(&src_mark[sl], -1, CLAIMED) == -1;
            // the winner's key goes to the slot of its own entry: entries in front of the item + the entry's place in the row
            const int64_t pos = (int64_t)a.entry_off[j] + (p - tr.indptr[row]);
            if (won && pos < a.cand_cap) a.cand[pos] = make_key(tr.src_type, sl);        // (pos < the level's entries = cand_cap)
        } else if (k) {
            const int64_t pos = (int64_t)base + kept + __popcll(mask & ((1ull << lane) - 1ull));
            if (pos < a.edge_cap) {                                     // (kept entries <= the level's entries <= edge_cap)
                a.src[pos] = src_mark[sl];
                a.dst[pos] = a.row_base + lrow;
                a.etype[pos] = tr.rel_id;
                if (a.etime) {
                    const int64_t dt = entry_time_diff(tr, row, sl);
                    if (dt < 0 || dt >= HGT_RTE_LEN) bad = true;
                    a.etime[pos] = dt;
                }
            }
        }
        kept += __popcll(mask);
    }
    if (!FILL) {
        if (lane == 0) a.chunk_cnt[c] = kept;
    } else if (__ballot(bad) != 0ull && lane == 0) {
        atomicOr((u64*)&a.head[H_FLAGS], (u64)HGT_NB_BAD_TIME);
    }
}

// the self loops of a bucket, behind its kept entries (head[H_KEPT], which the scan between the passes wrote)
__global__ __launch_bounds__(BS) void k_nb_self(const int64_t* __restrict__ head, int64_t n_level, int64_t row_base, int32_t rel_self,
                                                int64_t* __restrict__ src, int64_t* __restrict__ dst, int64_t* __restrict__ etype,
                                                int64_t* __restrict__ etime, int64_t edge_cap) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (i >= n_level) return;
    const int64_t pos = head[H_KEPT] + i;
    if (pos >= edge_cap) return;
    src[pos] = row_base + i;
    dst[pos] = row_base + i;
    etype[pos] = rel_self;
    if (etime) etime[pos] = HGT_RTE_SELF;
}

// one wavefront per result row: its feature row from its type's matrix
__global__ __launch_bounds__(BS) void k_nb_gather(const hgt_nb_type* __restrict__ types, const int64_t* __restrict__ node_type,
                                                  const int64_t* __restrict__ row_id, int64_t n_rows, int32_t width, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const hgt_nb_type ty = types[node_type[r]];
    const float* __restrict__ x = ty.feat + row_id[r] * ty.ld;
    float* __restrict__ y = out + r * (int64_t)width;
    for (int32_t cidx = lane; cidx < width; cidx += 64) y[cidx] = x[cidx];
}

__global__ __launch_bounds__(BS) void k_nb_out_rows(const hgt_nb_type* __restrict__ types, int32_t T, const int32_t* __restrict__ seed_type,
                                                    const int64_t* __restrict__ seed_id, int64_t S, int64_t* __restrict__ out_rows) {
    const int64_t s = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (s >= S) return;
    const int32_t t = seed_type[s];
    const int64_t id = seed_id[s];
    out_rows[s] = (t < 0 || t >= T || id < 0 || id >= types[t].n_nodes) ? -1 : types[t].mark[id];
}

__global__ __launch_bounds__(BS) void k_nb_reset(const hgt_nb_type* __restrict__ types, int32_t T, const uint64_t* __restrict__ keys, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    if (key == PAD_KEY) return;
    const int32_t t = (int32_t)(key >> 32), id = (int32_t)(uint32_t)key;
    if (t >= 0 && t < T && id >= 0 && id < types[t].n_nodes) types[t].mark[id] = -1;
}

static int key_bits(int32_t T) {
    int b = 0;
    while ((1 << b) < T) ++b;
    return 32 + (b > 0 ? b : 1);
}

static int check_tables(const void* types, int32_t T, const void* tri, int32_t M) {
    if (!types || T < 1 || T > MAX_T || M < 0 || M > MAX_M || (M > 0 && !tri)) return HGT_ERR_INVALID_ARG;
    return HGT_OK;
}

// the level's items from its rows per type (host arrays): HGT_ERR_INVALID_ARG unless 0 <= begin <= end <= n_level and all fits int32
static int make_items(const hgt_nb_triple* tri_types, int32_t M, int32_t T, const int64_t* type_begin, const int64_t* type_end,
                      int64_t n_level, ItemTab& it) {
    if (M > 0 && (!tri_types || !type_begin || !type_end)) return HGT_ERR_INVALID_ARG;
    int64_t n = 0;
    it.M = M;
    for (int m = 0; m < M; ++m) {
        const int32_t t = tri_types[m].tgt_type;
        if (t < 0 || t >= T || tri_types[m].src_type < 0 || tri_types[m].src_type >= T) return HGT_ERR_INVALID_ARG;
        if (type_begin[t] < 0 || type_end[t] < type_begin[t] || type_end[t] > n_level) return HGT_ERR_INVALID_ARG;
        it.base[m] = (int32_t)n;
        it.row0[m] = (int32_t)type_begin[t];
        n += type_end[t] - type_begin[t];
        if (n >= LIMIT) return HGT_ERR_INVALID_ARG;
    }
    it.base[M] = (int32_t)n;
    it.n_items = (int32_t)n;
    return HGT_OK;
}

}  // namespace

extern "C" int hgt_nb_constants(int32_t* chunk, int32_t* wave_rows, int32_t* head_words) {
    if (!chunk || !wave_rows || !head_words) return HGT_ERR_INVALID_ARG;
    *chunk = CHUNK; *wave_rows = HGT_NB_WAVE_ROWS; *head_words = HGT_NB_HEAD_WORDS;
    return HGT_OK;
}

extern "C" int hgt_nb_sort_bytes(int64_t capacity, int32_t n_types, uint64_t* bytes_host) {
    if (!bytes_host || capacity < 0 || capacity >= LIMIT || n_types < 1 || n_types > MAX_T) return HGT_ERR_INVALID_ARG;
    size_t b = 0;
    uint64_t* kp = nullptr;
    if (rocprim::radix_sort_keys(nullptr, b, kp, kp, (size_t)(capacity > 0 ? capacity : 1), 0, key_bits(n_types), (hipStream_t)0) != hipSuccess)
        return HGT_ERR_LAUNCH;
    *bytes_host = hgt_align_up((uint64_t)b + 256, 256);
    return HGT_OK;
}

extern "C" int hgt_nb_seeds(const hgt_nb_type* types_dev, int32_t n_types, const int32_t* seed_type, const int64_t* seed_id,
                            int64_t n_seeds, uint64_t* cand, int64_t* head, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (check_tables(types_dev, n_types, nullptr, 0) != HGT_OK || !head) return HGT_ERR_INVALID_ARG;
    if (n_seeds < 0 || n_seeds >= LIMIT || (n_seeds > 0 && (!seed_type || !seed_id || !cand))) return HGT_ERR_INVALID_ARG;
    k_nb_head_set<<<1, 64, 0, stream>>>(head, 0);
    if (n_seeds > 0) {
        if (hipMemsetAsync(cand, 0xFF, (size_t)n_seeds * 8, stream) != hipSuccess) return HGT_ERR_LAUNCH;
        k_nb_seeds<<<nblk(n_seeds, BS), BS, 0, stream>>>(types_dev, n_types, seed_type, seed_id, n_seeds, cand, head);
    }
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_nb_number(const hgt_nb_type* types_dev, int32_t n_types, const hgt_nb_triple* triples_dev, int32_t n_triples,
                             const uint64_t* cand, int64_t capacity, uint64_t* keys_out, void* sort_tmp, uint64_t sort_bytes,
                             int64_t row_base, int32_t expand, int64_t* order_out, int64_t* node_type_out, int64_t* row_id_out,
                             int64_t* head, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (check_tables(types_dev, n_types, triples_dev, n_triples) != HGT_OK || !head) return HGT_ERR_INVALID_ARG;
    if (capacity < 1 || capacity >= LIMIT || row_base < 0 || row_base + capacity >= LIMIT) return HGT_ERR_INVALID_ARG;
    if (!cand || !keys_out || !sort_tmp || !order_out || !node_type_out || !row_id_out) return HGT_ERR_INVALID_ARG;
    if (sort_bytes < 256) return HGT_ERR_WORKSPACE;                    // (below every answer of hgt_nb_sort_bytes: needs no size query)
    uint64_t need = 0;
    const int rc = hgt_nb_sort_bytes(capacity, n_types, &need);
    if (rc != HGT_OK) return rc;
    if (sort_bytes < need) return HGT_ERR_WORKSPACE;
    size_t bytes = (size_t)sort_bytes;
    if (rocprim::radix_sort_keys(sort_tmp, bytes, cand, keys_out, (size_t)capacity, 0, key_bits(n_types), stream) != hipSuccess)
        return HGT_ERR_LAUNCH;
    k_nb_head_set<<<1, 64, 0, stream>>>(head, 2);
    k_nb_number<<<nblk(capacity, BS), BS, 0, stream>>>(types_dev, triples_dev, n_triples, keys_out, capacity, row_base, expand ? 1 : 0,
                                                       order_out, node_type_out, row_id_out, head);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

static int walk_args(const hgt_nb_type* types_dev, int32_t n_types, const hgt_nb_triple* triples_dev,
                     const hgt_nb_triple* triples_host, int32_t n_triples, const uint64_t* keys, const int64_t* type_begin_host,
                     const int64_t* type_end_host, int64_t n_level, int64_t n_chunks, int32_t* item_chunks, int32_t* chunk_cnt,
                     int64_t* head, ItemTab& it) {
    if (check_tables(types_dev, n_types, triples_dev, n_triples) != HGT_OK || !head) return HGT_ERR_INVALID_ARG;
    if (n_level < 0 || n_level >= LIMIT || n_chunks < 0 || n_chunks >= LIMIT) return HGT_ERR_INVALID_ARG;
    const int rc = make_items(triples_host, n_triples, n_types, type_begin_host, type_end_host, n_level, it);
    if (rc != HGT_OK) return rc;
    if (n_chunks > 0 && (it.n_items == 0 || !keys || !item_chunks || !chunk_cnt)) return HGT_ERR_INVALID_ARG;
    return HGT_OK;
}

extern "C" int hgt_nb_expand(const hgt_nb_type* types_dev, int32_t n_types, const hgt_nb_triple* triples_dev,
                             const hgt_nb_triple* triples_host, int32_t n_triples, const uint64_t* keys,
                             const int64_t* type_begin_host, const int64_t* type_end_host, int64_t n_level, int64_t n_chunks,
                             int32_t has_max_time, int32_t max_time, int32_t* item_chunks, int32_t* item_entries, int32_t* chunk_cnt,
                             uint64_t* cand, int64_t capacity, int64_t* head, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ItemTab it;
    const int rc = walk_args(types_dev, n_types, triples_dev, triples_host, n_triples, keys, type_begin_host, type_end_host, n_level,
                             n_chunks, item_chunks, chunk_cnt, head, it);
    if (rc != HGT_OK) return rc;
    if (capacity < 0 || capacity >= LIMIT || (n_chunks > 0 && (!cand || !item_entries || capacity < 1))) return HGT_ERR_INVALID_ARG;
    k_nb_head_set<<<1, 64, 0, stream>>>(head, 1);
    if (n_chunks > 0) {
        if (hipMemsetAsync(cand, 0xFF, (size_t)capacity * 8, stream) != hipSuccess) return HGT_ERR_LAUNCH;
        k_nb_items<<<nblk(it.n_items, BS), BS, 0, stream>>>(triples_dev, it, keys, item_chunks, item_entries);
        k_nb_scan<<<1, SCAN_BS, 0, stream>>>(item_chunks, it.n_items, nullptr);
        k_nb_scan<<<1, SCAN_BS, 0, stream>>>(item_entries, it.n_items, nullptr);
        WalkArgs a{};
        a.types = types_dev; a.tri = triples_dev; a.keys = keys; a.item_off = item_chunks; a.chunk_cnt = chunk_cnt; a.n_chunks = n_chunks;
        a.has_max_time = has_max_time ? 1 : 0; a.max_time = max_time; a.head = head; a.cand = cand; a.cand_cap = capacity;
        a.entry_off = item_entries;
        k_nb_walk<false><<<nblk(n_chunks, BS / 64), BS, 0, stream>>>(a, it);
        k_nb_scan<<<1, SCAN_BS, 0, stream>>>(chunk_cnt, n_chunks, head + H_KEPT);
    }
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_nb_fill(const hgt_nb_type* types_dev, int32_t n_types, const hgt_nb_triple* triples_dev,
                           const hgt_nb_triple* triples_host, int32_t n_triples, const uint64_t* keys,
                           const int64_t* type_begin_host, const int64_t* type_end_host, int64_t n_level, int64_t n_chunks,
                           int32_t has_max_time, int32_t max_time, int32_t has_time, int32_t self_loops, int32_t rel_self, int64_t row_base,
                           const int32_t* item_chunks, int32_t* chunk_cnt, int64_t* src_out, int64_t* dst_out, int64_t* edge_type_out,
                           int64_t* edge_time_out, int64_t edge_capacity, int64_t* head, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ItemTab it;
    const int rc = walk_args(types_dev, n_types, triples_dev, triples_host, n_triples, keys, type_begin_host, type_end_host, n_level,
                             n_chunks, (int32_t*)item_chunks, chunk_cnt, head, it);
    if (rc != HGT_OK) return rc;
    if (edge_capacity < 0 || edge_capacity >= LIMIT || row_base < 0 || row_base + n_level >= LIMIT) return HGT_ERR_INVALID_ARG;
    const bool any = n_chunks > 0 || (self_loops && n_level > 0);
    if (any && (!src_out || !dst_out || !edge_type_out || (has_time && !edge_time_out))) return HGT_ERR_INVALID_ARG;
    if (self_loops && edge_capacity < n_level) return HGT_ERR_INVALID_ARG;
    if (n_chunks > 0) {
        WalkArgs a{};
        a.types = types_dev; a.tri = triples_dev; a.keys = keys; a.item_off = item_chunks; a.chunk_cnt = chunk_cnt; a.n_chunks = n_chunks;
        a.has_max_time = has_max_time ? 1 : 0; a.max_time = max_time; a.head = head; a.row_base = row_base;
        a.src = src_out; a.dst = dst_out; a.etype = edge_type_out; a.etime = has_time ? edge_time_out : nullptr; a.edge_cap = edge_capacity;
        k_nb_walk<true><<<nblk(n_chunks, BS / 64), BS, 0, stream>>>(a, it);
    }
    if (self_loops && n_level > 0)
        k_nb_self<<<nblk(n_level, BS), BS, 0, stream>>>(head, n_level, row_base, rel_self, src_out, dst_out, edge_type_out,
                                                        has_time ? edge_time_out : nullptr, edge_capacity);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_nb_finish(const hgt_nb_type* types_dev, int32_t n_types, const int64_t* node_type, const int64_t* row_id, int64_t n_rows,
                             int32_t width, float* feature_out, const int32_t* seed_type, const int64_t* seed_id, int64_t n_seeds,
                             int64_t* out_rows, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (check_tables(types_dev, n_types, nullptr, 0) != HGT_OK) return HGT_ERR_INVALID_ARG;
    if (n_rows < 0 || n_rows >= LIMIT || n_seeds < 0 || n_seeds >= LIMIT || width < 0) return HGT_ERR_INVALID_ARG;
    if (n_rows > 0 && width > 0 && (!node_type || !row_id || !feature_out)) return HGT_ERR_INVALID_ARG;
    if (n_seeds > 0 && (!seed_type || !seed_id || !out_rows)) return HGT_ERR_INVALID_ARG;
    if (n_rows > 0 && width > 0)
        k_nb_gather<<<nblk(n_rows, BS / 64), BS, 0, stream>>>(types_dev, node_type, row_id, n_rows, width, feature_out);
    if (n_seeds > 0) k_nb_out_rows<<<nblk(n_seeds, BS), BS, 0, stream>>>(types_dev, n_types, seed_type, seed_id, n_seeds, out_rows);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_nb_reset(const hgt_nb_type* types_dev, int32_t n_types, const uint64_t* keys, int64_t n, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (check_tables(types_dev, n_types, nullptr, 0) != HGT_OK || n < 0 || n >= LIMIT || (n > 0 && !keys)) return HGT_ERR_INVALID_ARG;
    if (n > 0) k_nb_reset<<<nblk(n, BS), BS, 0, stream>>>(types_dev, n_types, keys, n);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}
