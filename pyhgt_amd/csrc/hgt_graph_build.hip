// Building the resident graph from raw edge lists: (row ids, neighbour ids, times) of one direction of one relation -> the CSR
// (indptr, nbr, time) the reference's nested dicts would hold (ogbn-mag/preprocess_ogbn_mag.py:29-42, `elist[t_id][s_id] = year`), and
// the row means over CSR neighbourhoods of its lines 69-99.  include/hgt_hip.h states the contract; the numpy definitions are
// pyhgt_amd.graph_build.np_edge_lists_to_csr / np_neighbour_mean.
//
// The dict rule, per relation and direction:  a row's neighbours stand in the order of their FIRST entry, a repeated (row, neighbour)
// pair keeps that position and takes the time of its LAST entry.  On the device:
//   1  key[e] = (row << bits(n_nbrs)) | nbr, stable radix sort of (key, e): the copies of a pair are adjacent, in entry order
//   2  per sorted position: the head of a run marks keep[its entry] = 1, every other copy 0; the tail of a run writes the time of ITS
//      entry to tl[the head's entry] (a run of one is its own head; a longer run finds its head by a lower bound over the sorted keys --
//      repeats are the exception in the data this is for, so no pass over all entries is spent on them)
//   3  stable radix sort of (row, e): entry order inside a row = order of first appearance among the kept entries
//   4  flags in that order, an exclusive scan, one compaction; indptr[r] = scan[lower bound of r]
// Integers only; the one atomic is the OR into the error flag.  The sorts and the scan are rocPRIM's (as in hgt_plan.hip), the rest is
// hand-written.  Everything is enqueued on the caller's stream, nothing synchronises.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "hgt_graph_rule.h"

namespace {

constexpr int BS = 256;

static inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

static int key_bits(uint64_t n_values) {
    int b = 1;
    while (b < 32 && (1ull << b) < n_values) ++b;
    return b;
}

struct BuildLayout {
    uint64_t off_keys_in, off_keys_out, off_iota, off_vals_out, off_rows_in, off_keep, off_tl, off_sort_tmp, sort_tmp_bytes, total;
};

// rocPRIM's scratch for the two sorts and the scan.  rocPRIM derives it from the device it finds, so asking needs one; the size this
// library ASKS of its caller is host arithmetic (sort_tmp_bound: the ping-pong copies of the widest keys and of the values plus the
// histograms, with room to spare), and the build checks rocPRIM's answer against it before the first launch.
static uint64_t sort_tmp_bound(int64_t E) { return (uint64_t)E * 16 + (4ull << 20); }

static int sort_tmp_query(int64_t E, uint64_t* bytes) {
    size_t a = 0, b = 0, c = 0;
    uint64_t* k64 = nullptr;
    uint32_t* k32 = nullptr;
    int32_t* vp = nullptr;
    const size_t n = (size_t)(E > 0 ? E : 1);
    if (rocprim::radix_sort_pairs(nullptr, a, k64, k64, vp, vp, n, 0, 64, (hipStream_t)0) != hipSuccess) return HGT_ERR_LAUNCH;
    if (rocprim::radix_sort_pairs(nullptr, b, k32, k32, vp, vp, n, 0, 32, (hipStream_t)0) != hipSuccess) return HGT_ERR_LAUNCH;
    if (rocprim::exclusive_scan(nullptr, c, vp, vp, 0, n + 1, rocprim::plus<int32_t>(), (hipStream_t)0) != hipSuccess) return HGT_ERR_LAUNCH;
    size_t m = a > b ? a : b;
    m = m > c ? m : c;
    *bytes = (uint64_t)m + 256;
    return HGT_OK;
}

static BuildLayout build_layout(int64_t E, uint64_t sort_tmp_bytes) {
    BuildLayout t;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { uint64_t r = o; o = hgt_align_up(o + bytes, 256); return r; };
    const uint64_t n = (uint64_t)E;
    t.off_keys_in = take(n * 8);              // after sort 1: the sorted row keys (first half) and the row-sorted entries (second half)
    t.off_keys_out = take((n + 1) * 8);       // after step 2: flags int32[E + 1] and their scan int32[E + 1]
    t.off_iota = take(n * 4);
    t.off_vals_out = take(n * 4);
    t.off_rows_in = take(n * 4);
    t.off_keep = take(n * 4);
    t.off_tl = take(n * 4);
    t.sort_tmp_bytes = sort_tmp_bytes;
    t.off_sort_tmp = take(sort_tmp_bytes);
    t.total = o;
    return t;
}

__global__ void k_build_init(int32_t* __restrict__ indptr, int64_t n_rows, int32_t* __restrict__ status, int zero_indptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2) status[i] = 0;
    if (zero_indptr && i <= n_rows) indptr[i] = 0;
}

template <typename I>
__device__ __forceinline__ uint32_t read_id(const I* __restrict__ p, int64_t e, int64_t stride, int64_t n, bool& bad) {
    const int64_t v = (int64_t)p[e * stride];
    if (v < 0 || v >= n) { bad = true; return 0u; }
    return (uint32_t)v;
}

template <typename I>
__global__ void k_pair_keys(const I* __restrict__ rows, int64_t rs, const I* __restrict__ nbrs, int64_t ns, int64_t E, int64_t n_rows,
                            int64_t n_nbrs, int nb, uint64_t* __restrict__ keys, int32_t* __restrict__ iota,
                            uint32_t* __restrict__ row_keys, int32_t* __restrict__ status) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    bool bad = false;
    const uint32_t r = read_id(rows, e, rs, n_rows, bad);
    const uint32_t s = read_id(nbrs, e, ns, n_nbrs, bad);
    if (bad) atomicOr(&status[1], HGT_GRAPH_BAD_ID);
    keys[e] = ((uint64_t)r << nb) | (uint64_t)s;
    iota[e] = (int32_t)e;
    row_keys[e] = r;
}

// step 2 over the sorted positions
__global__ void k_mark(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t E, int nb,
                       const int32_t* __restrict__ edge_time, const int32_t* __restrict__ node_time, int by_nbr,
                       int32_t* __restrict__ keep, int32_t* __restrict__ tl) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const uint64_t key = keys[p];
    const bool head = p == 0 || keys[p - 1] != key;
    const bool tail = p == E - 1 || keys[p + 1] != key;
    const int32_t e = vals[p];
    keep[e] = head ? 1 : 0;
    if (!tail) return;
    int32_t tm = HGT_TIME_NONE;
    if (edge_time) tm = edge_time[e];
    else if (node_time) tm = node_time[by_nbr ? (uint32_t)(key & ((1ull << nb) - 1)) : (uint32_t)(key >> nb)];
    int64_t h = p;
    if (!head) {
        int64_t lo = 0, hi = p;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        h = lo;
    }
    tl[vals[h]] = tm;
}

__global__ void k_flags(const int32_t* __restrict__ by_row, const int32_t* __restrict__ keep, int64_t E, int32_t* __restrict__ flags) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > E) return;
    flags[q] = q < E ? keep[by_row[q]] : 0;
}

template <typename I>
__global__ void k_compact(const I* __restrict__ nbrs, int64_t ns, int64_t n_nbrs, const int32_t* __restrict__ by_row,
                          const int32_t* __restrict__ flags, const int32_t* __restrict__ pos, const int32_t* __restrict__ tl, int64_t E,
                          int32_t* __restrict__ nbr_out, int32_t* __restrict__ time_out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= E || !flags[q]) return;
    const int32_t e = by_row[q];
    bool bad = false;
    const int32_t o = pos[q];                 // < the number of kept entries <= E
    nbr_out[o] = (int32_t)read_id(nbrs, (int64_t)e, ns, n_nbrs, bad);
    time_out[o] = tl[e];
}

__global__ void k_indptr(const uint32_t* __restrict__ rows_sorted, const int32_t* __restrict__ pos, int64_t E, int64_t n_rows,
                         int32_t* __restrict__ indptr, int32_t* __restrict__ status) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rows) return;
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)rows_sorted[mid] < r) lo = mid + 1; else hi = mid;
    }
    indptr[r] = pos[lo];
    if (r == n_rows) status[0] = pos[E];
}

template <typename I>
static int build_impl(const I* rows, int64_t rs, const I* nbrs, int64_t ns, const int32_t* edge_time, const int32_t* node_time,
                      int by_nbr, int64_t E, int64_t n_rows, int64_t n_nbrs, int32_t* indptr, int32_t* nbr_out, int32_t* time_out,
                      int32_t* status, char* ws, const BuildLayout& L, hipStream_t stream) {
    uint64_t* keys_in = (uint64_t*)(ws + L.off_keys_in);
    uint64_t* keys_out = (uint64_t*)(ws + L.off_keys_out);
    int32_t* iota = (int32_t*)(ws + L.off_iota);
    int32_t* vals_out = (int32_t*)(ws + L.off_vals_out);
    uint32_t* rows_in = (uint32_t*)(ws + L.off_rows_in);
    int32_t* keep = (int32_t*)(ws + L.off_keep);
    int32_t* tl = (int32_t*)(ws + L.off_tl);
    void* sort_tmp = (void*)(ws + L.off_sort_tmp);
    uint32_t* rows_sorted = (uint32_t*)keys_in;                       // both valid once sort 1 has consumed keys_in
    int32_t* by_row = (int32_t*)(ws + L.off_keys_in) + E;
    int32_t* flags = (int32_t*)keys_out;                              // both valid once k_mark has consumed keys_out
    int32_t* pos = flags + (E + 1);
    const int nb = key_bits((uint64_t)n_nbrs), rb = key_bits((uint64_t)n_rows);

    k_build_init<<<1, 64, 0, stream>>>(indptr, n_rows, status, 0);
    k_pair_keys<I><<<nblk(E, BS), BS, 0, stream>>>(rows, rs, nbrs, ns, E, n_rows, n_nbrs, nb, keys_in, iota, rows_in, status);
    size_t sort_bytes = (size_t)L.sort_tmp_bytes;
    if (rocprim::radix_sort_pairs(sort_tmp, sort_bytes, keys_in, keys_out, iota, vals_out, (size_t)E, 0, nb + rb, stream) != hipSuccess)
        return HGT_ERR_LAUNCH;
    k_mark<<<nblk(E, BS), BS, 0, stream>>>(keys_out, vals_out, E, nb, edge_time, node_time, by_nbr, keep, tl);
    sort_bytes = (size_t)L.sort_tmp_bytes;
    if (rocprim::radix_sort_pairs(sort_tmp, sort_bytes, rows_in, rows_sorted, iota, by_row, (size_t)E, 0, rb, stream) != hipSuccess)
        return HGT_ERR_LAUNCH;
    k_flags<<<nblk(E + 1, BS), BS, 0, stream>>>(by_row, keep, E, flags);
    sort_bytes = (size_t)L.sort_tmp_bytes;
    if (rocprim::exclusive_scan(sort_tmp, sort_bytes, flags, pos, 0, (size_t)(E + 1), rocprim::plus<int32_t>(), stream) != hipSuccess)
        return HGT_ERR_LAUNCH;
    k_compact<I><<<nblk(E, BS), BS, 0, stream>>>(nbrs, ns, n_nbrs, by_row, flags, pos, tl, E, nbr_out, time_out);
    k_indptr<<<nblk(n_rows + 1, BS), BS, 0, stream>>>(rows_sorted, pos, E, n_rows, indptr, status);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

// ------------------------------------------------------------------------------------------------------------- neighbour mean
// A row's terms are ONE sequence: the CSRs in table order, a CSR's neighbours in its order.  One wavefront adds the terms [p0, p1) of
// a row for one tile of 64 * VEC columns (blockIdx.y), term by term: the ids of 64 terms are read by the lanes at once and handed
// round with a shuffle, the gathered rows are loaded UNROLL at a time (independent loads in flight) and added in term order.
// VEC floats per lane and load: 4 for rows wider than 128 columns, 2 wider than 64 (one 512-byte row of d = 128 fills the wavefront
// with 8-byte loads), else 1 -- where x's base and row stride allow the width, scalar loads otherwise and in a row's ragged last lane.
struct MeanTable {
    const int32_t* indptr[HGT_SAMPLER_MAX_TRIPLES];
    const int32_t* nbr[HGT_SAMPLER_MAX_TRIPLES];
    int n;
};
struct MeanLong { int32_t row, base, n_chunks, count; };
struct MeanItem { int32_t row, chunk; };
constexpr int UNROLL = 4;

template <int VEC>
struct Acc { float v[VEC]; };

template <int VEC>
__device__ __forceinline__ Acc<VEC> load_row(const float* __restrict__ x, int64_t ldx, int32_t id, int col, int nv, bool wide) {
    Acc<VEC> a;
    const float* p = x + (int64_t)id * ldx + col;
    if (VEC == 4 && wide && nv == 4) {
        const float4 t = *(const float4*)p;
        a.v[0] = t.x; a.v[1 % VEC] = t.y; a.v[2 % VEC] = t.z; a.v[3 % VEC] = t.w;
    } else if (VEC == 2 && wide && nv == 2) {
        const float2 t = *(const float2*)p;
        a.v[0] = t.x; a.v[1 % VEC] = t.y;
    } else {
#pragma unroll
        for (int u = 0; u < VEC; ++u) a.v[u] = u < nv ? p[u] : 0.0f;
    }
    return a;
}

// acc += the terms [p0, p1) of row `row`'s sequence; every lane of the wavefront calls it with the same (row, p0, p1)
template <int VEC>
__device__ __forceinline__ void add_terms(const MeanTable& tab, const float* __restrict__ x, int64_t ldx, int row, int64_t p0, int64_t p1,
                                          int col, int nv, bool wide, Acc<VEC>& acc) {
    const int lane = threadIdx.x & 63;
    int64_t off = 0;
    for (int m = 0; m < tab.n && off < p1; ++m) {
        const int b = tab.indptr[m][row], e = tab.indptr[m][row + 1];
        const int64_t len = e - b;
        const int64_t lo = p0 > off ? p0 - off : 0, hi = (p1 - off) < len ? (p1 - off) : len;
        const int32_t* __restrict__ nbr = tab.nbr[m] + b;
        for (int64_t j = lo; j < hi; j += 64) {
            const int cnt = (int)((hi - j) < 64 ? (hi - j) : 64);
            const int32_t mine = lane < cnt ? nbr[j + lane] : 0;
            int u = 0;
            for (; u + UNROLL <= cnt; u += UNROLL) {
                Acc<VEC> t[UNROLL];
#pragma unroll
                for (int w = 0; w < UNROLL; ++w) t[w] = load_row<VEC>(x, ldx, __shfl(mine, u + w), col, nv, wide);
#pragma unroll
                for (int w = 0; w < UNROLL; ++w)
#pragma unroll
                    for (int c = 0; c < VEC; ++c) acc.v[c] += t[w].v[c];
            }
            for (; u < cnt; ++u) {
                const Acc<VEC> t = load_row<VEC>(x, ldx, __shfl(mine, u), col, nv, wide);
#pragma unroll
                for (int c = 0; c < VEC; ++c) acc.v[c] += t.v[c];
            }
        }
        off += len;
    }
}

template <int VEC>
__device__ __forceinline__ void store_row(float* __restrict__ p, const Acc<VEC>& a, int nv) {
#pragma unroll
    for (int u = 0; u < VEC; ++u)
        if (u < nv) p[u] = a.v[u];
}

// one wavefront per (row, column tile): short rows are finished here; a long row is entered into the chunk list by its tile-0 wavefront
// (the slots come from an integer counter: which slots a row gets does not show in the output)
template <int VEC>
__global__ __launch_bounds__(256) void k_mean_rows(MeanTable tab, const float* __restrict__ x, int64_t ldx, int64_t n_rows, int d, bool wide,
                                                   float* __restrict__ out, int64_t ldo, int32_t* __restrict__ counters,
                                                   MeanLong* __restrict__ longs, int64_t max_long, MeanItem* __restrict__ items,
                                                   int64_t max_items) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int col = (blockIdx.y * 64 + lane) * VEC;
    const int nv = d - col < 0 ? 0 : (d - col < VEC ? d - col : VEC);
    int64_t k = 0;
    for (int m = 0; m < tab.n; ++m) k += tab.indptr[m][row + 1] - tab.indptr[m][row];
    if (k > HGT_GRAPH_MEAN_CHUNK) {
        if (blockIdx.y != 0) return;
        const int nch = (int)((k + HGT_GRAPH_MEAN_CHUNK - 1) / HGT_GRAPH_MEAN_CHUNK);
        int base = 0, slot = 0;
        if (lane == 0) { base = atomicAdd(&counters[0], nch); slot = atomicAdd(&counters[1], 1); }
        base = __shfl(base, 0);
        slot = __shfl(slot, 0);
        if ((int64_t)base + nch > max_items || slot >= max_long) return;      // cannot happen with CSRs whose lengths sum to n_entries
        if (lane == 0) longs[slot] = MeanLong{(int32_t)row, base, nch, (int32_t)k};
        for (int c = lane; c < nch; c += 64) items[base + c] = MeanItem{(int32_t)row, c};
        return;
    }
    Acc<VEC> acc;
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc.v[c] = 0.0f;
    add_terms<VEC>(tab, x, ldx, (int)row, 0, k, col, nv, wide, acc);
    if (k > 0) {
        const float kf = (float)k;
#pragma unroll
        for (int c = 0; c < VEC; ++c) acc.v[c] = acc.v[c] / kf;
    }
    if (nv > 0) store_row<VEC>(out + row * ldo + col, acc, nv);
}

template <int VEC>
__global__ __launch_bounds__(256) void k_mean_chunks(MeanTable tab, const float* __restrict__ x, int64_t ldx, int d, bool wide,
                                                     const int32_t* __restrict__ counters, const MeanItem* __restrict__ items,
                                                     int64_t max_items, int64_t n_rows, float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_items = counters[0] < max_items ? counters[0] : max_items;
    if (it >= n_items) return;
    const int col = (blockIdx.y * 64 + lane) * VEC;
    const int nv = d - col < 0 ? 0 : (d - col < VEC ? d - col : VEC);
    const MeanItem item = items[it];
    if (item.row < 0 || item.row >= n_rows || item.chunk < 0) return;      // a slot k_mean_rows refused to fill (see its guard)
    Acc<VEC> acc;
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc.v[c] = 0.0f;
    const int64_t p0 = (int64_t)item.chunk * HGT_GRAPH_MEAN_CHUNK;
    add_terms<VEC>(tab, x, ldx, item.row, p0, p0 + HGT_GRAPH_MEAN_CHUNK, col, nv, wide, acc);   // add_terms stops at the row's end
    if (nv > 0) store_row<VEC>(partial + it * (int64_t)d + col, acc, nv);
}

// one thread per (long row, column): the chunk sums in chunk order, then the division
__global__ void k_mean_join(const int32_t* __restrict__ counters, const MeanLong* __restrict__ longs, int64_t max_long, int64_t max_items,
                            const float* __restrict__ partial, int d, float* __restrict__ out, int64_t ldo) {
    const int64_t n_long = counters[1] < max_long ? counters[1] : max_long;
    const int64_t li = blockIdx.x;
    if (li >= n_long) return;
    const MeanLong L = longs[li];
    if ((int64_t)L.base + L.n_chunks > max_items) return;
    const float kf = (float)L.count;
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        float acc = partial[(int64_t)L.base * d + c];
        for (int j = 1; j < L.n_chunks; ++j) acc += partial[(int64_t)(L.base + j) * d + c];
        out[(int64_t)L.row * ldo + c] = acc / kf;
    }
}

struct MeanLayout { uint64_t off_counters, off_longs, off_items, off_partial, total; int64_t max_long, max_items; };

static MeanLayout mean_layout(int64_t n_entries, int32_t d) {
    MeanLayout t;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { uint64_t r = o; o = hgt_align_up(o + bytes, 256); return r; };
    // a long row has more than CHUNK terms: fewer than n_entries / CHUNK of them, with at most n_entries / CHUNK + (their number) chunks
    t.max_long = n_entries / HGT_GRAPH_MEAN_CHUNK;
    t.max_items = 2 * t.max_long;
    t.off_counters = take(256);
    t.off_longs = take((uint64_t)t.max_long * sizeof(MeanLong));
    t.off_items = take((uint64_t)t.max_items * sizeof(MeanItem));
    t.off_partial = take((uint64_t)t.max_items * (uint64_t)d * 4);
    t.total = o;
    return t;
}

template <int VEC>
static void mean_launch(const MeanTable& tab, const float* x, int64_t ldx, int64_t n_rows, int32_t d, bool wide, float* out, int64_t ldo,
                        char* ws, const MeanLayout& L, hipStream_t stream) {
    int32_t* counters = (int32_t*)(ws + L.off_counters);
    MeanLong* longs = (MeanLong*)(ws + L.off_longs);
    MeanItem* items = (MeanItem*)(ws + L.off_items);
    float* partial = (float*)(ws + L.off_partial);
    const unsigned tiles = (unsigned)((d + 64 * VEC - 1) / (64 * VEC));
    k_mean_rows<VEC><<<dim3(nblk(n_rows, 4), tiles), 256, 0, stream>>>(tab, x, ldx, n_rows, d, wide, out, ldo, counters, longs, L.max_long,
                                                                       items, L.max_items);
    if (L.max_long > 0) {
        k_mean_chunks<VEC><<<dim3(nblk(L.max_items, 4), tiles), 256, 0, stream>>>(tab, x, ldx, d, wide, counters, items, L.max_items, n_rows,
                                                                                  partial);
        k_mean_join<<<(unsigned)L.max_long, 256, 0, stream>>>(counters, longs, L.max_long, L.max_items, partial, d, out, ldo);
    }
}

}  // namespace

extern "C" int hgt_graph_csr_bytes(int64_t E, uint64_t* ws_bytes_host) {
    if (!ws_bytes_host || E < 0) return HGT_ERR_INVALID_ARG;
    if (E >= (1ll << 31) - 1) return HGT_ERR_TOO_LARGE;
    *ws_bytes_host = build_layout(E, sort_tmp_bound(E)).total;
    return HGT_OK;
}

extern "C" int hgt_graph_csr_build(const void* rows, int64_t row_stride, const void* nbrs, int64_t nbr_stride, int32_t id_bytes,
                                   const int32_t* edge_time, const int32_t* node_time, int32_t node_time_by, int64_t E, int64_t n_rows,
                                   int64_t n_nbrs, int32_t* indptr, int32_t* nbr_out, int32_t* time_out, int32_t* status, void* ws,
                                   uint64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (E < 0 || n_rows < 0 || n_nbrs < 0 || row_stride < 0 || nbr_stride < 0 || (id_bytes != 4 && id_bytes != 8)) return HGT_ERR_INVALID_ARG;
    if (!indptr || !status || !ws || (edge_time && node_time)) return HGT_ERR_INVALID_ARG;
    if (node_time_by != HGT_GRAPH_TIME_BY_ROW && node_time_by != HGT_GRAPH_TIME_BY_NBR) return HGT_ERR_INVALID_ARG;
    if (E > 0 && (!rows || !nbrs || !nbr_out || !time_out || n_rows < 1 || n_nbrs < 1)) return HGT_ERR_INVALID_ARG;
    if (E >= (1ll << 31) - 1 || n_rows >= (1ll << 31) - 1 || n_nbrs >= (1ll << 31) - 1) return HGT_ERR_TOO_LARGE;
    const BuildLayout L = build_layout(E, sort_tmp_bound(E));
    if (ws_bytes < L.total) return HGT_ERR_WORKSPACE;
    uint64_t st = 0;
    const int rc = sort_tmp_query(E, &st);
    if (rc != HGT_OK) return rc;
    if (st > L.sort_tmp_bytes) return HGT_ERR_UNSUPPORTED;      // a rocPRIM whose sorts want more than this library reserves for them
    if (E == 0) {
        k_build_init<<<nblk(n_rows + 1 > 2 ? n_rows + 1 : 2, BS), BS, 0, stream>>>(indptr, n_rows, status, 1);
        HGT_CHECK_LAUNCH();
        return HGT_OK;
    }
    const int by_nbr = node_time_by == HGT_GRAPH_TIME_BY_NBR;
    if (id_bytes == 8)
        return build_impl<int64_t>((const int64_t*)rows, row_stride, (const int64_t*)nbrs, nbr_stride, edge_time, node_time, by_nbr, E, n_rows,
                                   n_nbrs, indptr, nbr_out, time_out, status, (char*)ws, L, stream);
    return build_impl<int32_t>((const int32_t*)rows, row_stride, (const int32_t*)nbrs, nbr_stride, edge_time, node_time, by_nbr, E, n_rows,
                               n_nbrs, indptr, nbr_out, time_out, status, (char*)ws, L, stream);
}

extern "C" int hgt_neighbour_mean_bytes(int64_t n_entries, int32_t d, uint64_t* ws_bytes_host) {
    if (!ws_bytes_host || n_entries < 0 || d < 1) return HGT_ERR_INVALID_ARG;
    if (n_entries >= (1ll << 31) - 1) return HGT_ERR_TOO_LARGE;
    *ws_bytes_host = mean_layout(n_entries, d).total;
    return HGT_OK;
}

extern "C" int hgt_neighbour_mean(const hgt_graph_csr* csrs_host, int32_t n_csr, const float* x, int64_t ldx, int64_t n_rows,
                                  int64_t n_entries, int32_t d, float* out, int64_t ldo, void* ws, uint64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!csrs_host || n_csr < 1 || d < 1 || n_rows < 0 || n_entries < 0 || ldx < d || ldo < d) return HGT_ERR_INVALID_ARG;
    if (n_csr > HGT_SAMPLER_MAX_TRIPLES) return HGT_ERR_UNSUPPORTED;
    if (n_rows >= (1ll << 31) - 1 || n_entries >= (1ll << 31) - 1) return HGT_ERR_TOO_LARGE;
    if (n_rows == 0) return HGT_OK;
    if (!out || !ws || (n_entries > 0 && !x)) return HGT_ERR_INVALID_ARG;
    MeanTable tab;
    tab.n = n_csr;
    for (int m = 0; m < n_csr; ++m) {
        if (!csrs_host[m].indptr || (n_entries > 0 && !csrs_host[m].nbr)) return HGT_ERR_INVALID_ARG;
        tab.indptr[m] = csrs_host[m].indptr;
        tab.nbr[m] = csrs_host[m].nbr;
    }
    const MeanLayout L = mean_layout(n_entries, d);
    if (ws_bytes < L.total) return HGT_ERR_WORKSPACE;
    if (hipMemsetAsync((char*)ws + L.off_counters, 0, 256, stream) != hipSuccess) return HGT_ERR_LAUNCH;
    const uintptr_t xa = (uintptr_t)x;
    if (d > 128) mean_launch<4>(tab, x, ldx, n_rows, d, xa % 16 == 0 && ldx % 4 == 0, out, ldo, (char*)ws, L, stream);
    else if (d > 64) mean_launch<2>(tab, x, ldx, n_rows, d, xa % 8 == 0 && ldx % 2 == 0, out, ldo, (char*)ws, L, stream);
    else mean_launch<1>(tab, x, ldx, n_rows, d, false, out, ldo, (char*)ws, L, stream);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}
