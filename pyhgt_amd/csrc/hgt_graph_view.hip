// Whole-graph view of a resident graph: the CSRs of every meta triple -> the reference's wire format (to_torch, pyHGT/data.py:212-256)
// over ALL nodes and ALL (or the kept) edges, in the sorted int32 form hgt_plan_from_sorted takes and as the int64 tensors the model is
// called with.  include/hgt_hip.h states the contract; the numpy definition is pyhgt_amd.view.np_whole_graph.
//
//   entry space   the concatenation of the triples' CSR entries in table order (relation id, then target type) and, last, one self
//                 entry per node.  Entry e of triple m is position p = e - first[m] of its CSR: source src_off + src[p], target
//                 tgt_off + row(p), relation rel_id.  The order of the kept entries IS the output order, so a kept entry's position is
//                 the number of kept entries in front of it -- one bucket, no sort.
//   tiles         HGT_VIEW_TILE consecutive entries belong to ONE wavefront, which takes them 64 at a time; a workgroup is four such
//                 wavefronts.  A wavefront finds the row of its first entry in a triple by one binary search of indptr and walks from
//                 there: it loads 64 row starts at a time and every lane counts the starts at or below its position with seven
//                 cross-lane reads.  A stretch of more than WALK_BATCHES * 64 rows without an entry falls back to a search per lane.
//   unfiltered    position = entry index: ONE launch.
//   filtered      count (kept entries per tile) -> one single-workgroup scan -> fill, where a kept entry's position = the scan's value
//                 for its tile + the kept entries of the wavefront's earlier steps + its rank in a ballot.  No position comes from an
//                 atomic: every output array is a function of the inputs alone.
//   rel_ptr       the lane that holds the first entry of a triple writes its own position for the relation ids that begin there;
//                 the ids behind the last entry get the total from workgroup 0.
// Integers only; the only atomic is the OR into the flag word.  Nothing synchronises: where the caller gives a pinned buffer (a filtered
// build's one host read), rel_ptr and the flag travel there with one hipMemcpyAsync on the caller's stream.
#include "hgt_graph_rule.h"

namespace {

constexpr int BS = 256;                                // four wavefronts, one tile each
constexpr int TILE = HGT_VIEW_TILE;                    // entries of one wavefront
constexpr int STEPS = TILE / 64;
constexpr int WALK_BATCHES = 4;                        // row starts looked at 64 at a time before the walk gives up
constexpr int SCAN_BS = 1024;
constexpr int64_t LIMIT = (1ll << 31) - 1;

struct ViewArgs {
    const hgt_view_triple* tab;                        // [M + 1] in device memory: the triples, then the self run
    int32_t M, R;
    int64_t E;                                         // entries of the whole entry space (self run included)
    int32_t has_max_time, max_time, has_time;
    int32_t* src32; int32_t* dst32; int32_t* time32;
    int64_t* ei; int64_t ei_stride; int64_t* etype; int64_t* etime;
    int32_t* rel_ptr;                                  // [R + 2]: rel_ptr[0..R], flag
    int32_t* cnt;                                      // [n_tiles + 1]: kept entries per tile, scanned in place (filtered views)
    int64_t n_tiles;
};

__device__ __forceinline__ int64_t tri_end(const ViewArgs& a, int m) { return m < a.M ? a.tab[m + 1].first : a.E; }

// the last row r in [0, n_rows) with indptr[r] <= p (indptr[0] = 0 <= p < indptr[n_rows])
__device__ __forceinline__ int32_t row_search(const int32_t* __restrict__ indptr, int32_t lo, int32_t n_rows, int32_t p) {
    int32_t hi = n_rows - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (indptr[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Rows of up to 64 consecutive positions of one CSR: lane `lane` of the `member` lanes holds position p; r0 is a row with
// indptr[r0] <= p for all of them.  -> the row of p.  Every lane of the wavefront takes part (the cross-lane reads need them all).
__device__ __forceinline__ int32_t rows_by_walk(const int32_t* __restrict__ indptr, int32_t n_rows, int32_t r0, int32_t p, bool member,
                                                int lane) {
    int32_t add = 0, rb = r0 + 1;
    for (int it = 0;; ++it) {
        const int64_t r = (int64_t)rb + lane;
        const int32_t b = r <= n_rows ? indptr[r] : INT32_MAX;       // (indptr has n_rows + 1 entries)
        int c = 0;                                                     // starts of this batch at or below p
        for (int s = 32; s >= 1; s >>= 1) {
            const int32_t v = __shfl(b, c + s - 1);
            if (v <= p) c += s;
        }
        if (__shfl(b, c) <= p) c += 1;                                 // c <= 63 here; 64 = the whole batch
        if (member) add += c;
        const bool more = member && c == 64;
        if (__ballot(more) == 0ull) break;
        rb += 64;                                                      // (rb + 63 <= n_rows here: a start above p ends the batch)
        if (it + 1 == WALK_BATCHES) {
            if (more) add = row_search(indptr, rb - 1, n_rows, p) - r0;
            break;
        }
    }
    return r0 + add;
}

// One wavefront's tile.  COUNT: -> the kept entries of the tile.  else: writes the outputs, positions from `base` on (FILTER) or the
// entry indices.
template <bool FILTER, bool COUNT>
__device__ __forceinline__ int32_t view_tile(const ViewArgs& a, int64_t w0, int32_t base, int lane, bool& bad) {
    const int M = a.M;
    int m = 0;
    int32_t prev_rel = -1;                                             // relation of the last triple in front that has entries
    while (m < M && a.tab[m + 1].first <= w0) {
        if (a.tab[m + 1].first > a.tab[m].first) prev_rel = a.tab[m].rel_id;
        ++m;
    }
    int32_t cursor = -1;                                               // row of the wavefront's last entry in triple m, -1: not known
    int32_t kept = 0;
    for (int step = 0; step < STEPS; ++step) {
        const int64_t e0 = w0 + step * 64;
        if (e0 >= a.E) break;
        const int64_t e = e0 + lane;
        const int64_t seg_end = e0 + 64 < a.E ? e0 + 64 : a.E;
        bool keep = false;
        int32_t s = 0, d = 0, t = HGT_RTE_SELF, rel = 0, rel_lo = 0, rel_hi = -1;
        int64_t cur = e0;
        while (cur < seg_end) {                                        // the triples this step touches (uniform over the wavefront)
            const hgt_view_triple tr = a.tab[m];
            const int64_t end = tri_end(a, m);
            if (end <= cur) {                                          // an empty triple
                ++m; cursor = -1;
                continue;
            }
            const int64_t hi = end < seg_end ? end : seg_end;
            const bool member = e >= cur && e < hi;
            if (cur == tr.first && e == cur) { rel_lo = prev_rel + 1; rel_hi = tr.rel_id; }
            if (m < M) {
                const int32_t p0 = (int32_t)(cur - tr.first);
                const int32_t p = member ? (int32_t)(e - tr.first) : p0;
                if (cursor < 0) cursor = row_search(tr.indptr, 0, tr.n_rows, p0);
                const int32_t row = rows_by_walk(tr.indptr, tr.n_rows, cursor, p, member, lane);
                cursor = __shfl(row, (int)(hi - 1 - e0));
                if (member) {
                    const int32_t sl = tr.src[p];
                    const bool k = !FILTER || entry_kept(tr, row, p, sl, a.has_max_time, a.max_time);
                    keep = k;
                    if (!COUNT) {
                        s = tr.src_off + sl; d = tr.tgt_off + row; rel = tr.rel_id;
                        if (tr.tgt_time) {
                            const int64_t dt = entry_time_diff(tr, row, sl);
                            if (k && (dt < 0 || dt >= HGT_RTE_LEN)) bad = true;
                            // written as it is (saturated to int32 only): the plan build and every layer that reads edge_time
                            // flag a value outside [0, 240) themselves, as they do for any caller's tensors
                            t = (int32_t)(dt < INT32_MIN ? INT32_MIN : dt > INT32_MAX ? INT32_MAX : dt);
                        }
                    }
                }
            } else if (member) {                                       // the self run: never filtered
                keep = true;
                s = d = (int32_t)(e - tr.first); rel = tr.rel_id; t = HGT_RTE_SELF;
            }
            cur = hi;
            if (hi == end) { prev_rel = tr.rel_id; ++m; cursor = -1; }
        }
        const unsigned long long mask = __ballot(keep);
        if (!COUNT) {
            const int64_t pos = FILTER ? (int64_t)base + kept + __popcll(mask & ((1ull << lane) - 1ull)) : e;
            for (int32_t r = rel_lo; r <= rel_hi; ++r) a.rel_ptr[r] = (int32_t)pos;      // (0 <= r < R: relation ids of the table)
            if (keep) {                                                // pos < kept total <= E = the arrays' capacity
                a.src32[pos] = s; a.dst32[pos] = d;
                if (a.time32) a.time32[pos] = t;
                if (a.ei) {
                    a.ei[pos] = s; a.ei[a.ei_stride + pos] = d; a.etype[pos] = rel;
                    if (a.etime) a.etime[pos] = t;
                }
            }
        }
        kept += __popcll(mask);
    }
    return kept;
}

__global__ __launch_bounds__(BS) void k_view_count(ViewArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;                                     // (a whole wavefront)
    bool bad = false;
    const int32_t kept = view_tile<true, true>(a, tile * TILE, 0, lane, bad);
    if (lane == 0) a.cnt[tile] = kept;
}

// exclusive scan of cnt[0, n] by ONE workgroup; cnt[n] becomes the total
__global__ __launch_bounds__(SCAN_BS) void k_view_scan(int32_t* __restrict__ cnt, int64_t n) {
    __shared__ int32_t wsum[SCAN_BS / 64];
    __shared__ int32_t carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { carry = 0; cnt[n] = 0; }
    __syncthreads();
    for (int64_t b0 = 0; b0 <= n; b0 += SCAN_BS) {
        const int64_t i = b0 + threadIdx.x;
        const int32_t v = i <= n ? cnt[i] : 0;
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
        if (i <= n) cnt[i] = c + before + x - v;
        __syncthreads();
        if (threadIdx.x == 0) carry = c + total;
        __syncthreads();
    }
}

template <bool FILTER>
__global__ __launch_bounds__(BS) void k_view_fill(ViewArgs a) {
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && (int)threadIdx.x <= a.R) {                  // the relation ids that begin behind the last entry
        int32_t last_rel = -1;
        for (int m = 0; m <= a.M; ++m)
            if (tri_end(a, m) > a.tab[m].first) last_rel = a.tab[m].rel_id;
        if ((int)threadIdx.x > last_rel) a.rel_ptr[threadIdx.x] = FILTER ? a.cnt[a.n_tiles] : (int32_t)a.E;
    }
    const int64_t tile = (int64_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;
    bool bad = false;
    view_tile<FILTER, false>(a, tile * TILE, FILTER ? a.cnt[tile] : 0, lane, bad);
    if (__ballot(bad) != 0ull && lane == 0) atomicOr(&a.rel_ptr[a.R + 1], HGT_VIEW_BAD_TIME);
}

static int check_sizes(int64_t n_entries, int32_t n_triples, int32_t n_relations) {
    if (n_entries < 0 || n_triples < 0 || n_relations < 1) return HGT_ERR_INVALID_ARG;
    if (n_entries >= LIMIT) return HGT_ERR_INVALID_ARG;
    if (n_triples > HGT_SAMPLER_MAX_TRIPLES || n_relations > HGT_SAMPLER_MAX_TRIPLES + 1) return HGT_ERR_INVALID_ARG;
    return HGT_OK;
}

static inline int64_t n_tiles_of(int64_t n_entries) { return (n_entries + TILE - 1) / TILE; }

}  // namespace

extern "C" int hgt_view_tmp_bytes(int64_t n_entries, uint64_t* tmp_bytes_host) {
    if (!tmp_bytes_host || n_entries < 0 || n_entries >= LIMIT) return HGT_ERR_INVALID_ARG;
    *tmp_bytes_host = hgt_align_up((uint64_t)(n_tiles_of(n_entries) + 1) * 4, 256);
    return HGT_OK;
}

extern "C" int hgt_view_build(const hgt_view_triple* table_dev, int32_t n_triples, int32_t n_relations, int64_t n_entries,
                              int32_t filtered, int32_t has_max_time, int32_t max_time, int32_t has_time, int32_t* src32,
                              int32_t* dst32, int32_t* time32, int64_t* edge_index, int64_t edge_index_stride, int64_t* edge_type,
                              int64_t* edge_time, int32_t* rel_ptr, void* tmp, uint64_t tmp_bytes, void* head_host_pinned,
                              void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check_sizes(n_entries, n_triples, n_relations);
    if (rc != HGT_OK) return rc;
    if (!table_dev || !rel_ptr) return HGT_ERR_INVALID_ARG;
    if (n_entries > 0 && (!src32 || !dst32 || (has_time && !time32))) return HGT_ERR_INVALID_ARG;
    if (n_entries > 0 && edge_index && (!edge_type || (has_time && !edge_time) || edge_index_stride < n_entries)) return HGT_ERR_INVALID_ARG;
    if (filtered && !tmp) return HGT_ERR_INVALID_ARG;
    const int64_t n_tiles = n_tiles_of(n_entries);
    if (filtered && tmp_bytes < (uint64_t)(n_tiles + 1) * 4) return HGT_ERR_WORKSPACE;
    ViewArgs a;
    a.tab = table_dev; a.M = n_triples; a.R = n_relations; a.E = n_entries;
    a.has_max_time = has_max_time ? 1 : 0; a.max_time = max_time; a.has_time = has_time ? 1 : 0;
    a.src32 = src32; a.dst32 = dst32; a.time32 = has_time ? time32 : nullptr;
    a.ei = edge_index; a.ei_stride = edge_index_stride; a.etype = edge_type; a.etime = has_time ? edge_time : nullptr;
    a.rel_ptr = rel_ptr; a.cnt = (int32_t*)tmp; a.n_tiles = n_tiles;
    if (hipMemsetAsync(rel_ptr + n_relations + 1, 0, 4, stream) != hipSuccess) return HGT_ERR_LAUNCH;
    const unsigned grid = (unsigned)((n_tiles + BS / 64 - 1) / (BS / 64));
    if (filtered) {
        if (grid > 0) k_view_count<<<grid, BS, 0, stream>>>(a);
        k_view_scan<<<1, SCAN_BS, 0, stream>>>(a.cnt, n_tiles);
        k_view_fill<true><<<grid > 0 ? grid : 1, BS, 0, stream>>>(a);
    } else {
        k_view_fill<false><<<grid > 0 ? grid : 1, BS, 0, stream>>>(a);
    }
    HGT_CHECK_LAUNCH();
    if (head_host_pinned &&
        hipMemcpyAsync(head_host_pinned, rel_ptr, (size_t)(n_relations + 2) * 4, hipMemcpyDeviceToHost, stream) != hipSuccess)
        return HGT_ERR_LAUNCH;
    return HGT_OK;
}
