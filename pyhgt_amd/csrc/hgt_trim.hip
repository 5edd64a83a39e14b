// Seed-trimmed graphs: (graph, seeds, L) -> the nested row and edge sets each layer of an L-layer stack needs for the seed rows, in
// hop-major order.  include/hgt_hip.h states the contract; the numpy definition is pyhgt_amd.trim.np_trim_to_seeds.
//
//   hops   hop[v] = L + 1 ("out"), 0 at the seeds; round r = 1..L, one launch each: every edge (s -> t) with hop[t] == r - 1 lowers
//          hop[s] to r (atomicMin: every writer of a round writes the same r, and a value r - 1 was final before the round began, so
//          neither the result nor what a round reads depends on arrival order).  The launch boundary is the only global synchronisation.
//   order  rows by (hop, old row) and edges by (hop[target], old position) are stable partitions into at most L + 2 buckets: a
//          workgroup counts its tile's keys per bucket (integer LDS atomics on a histogram: a count, not an order), ONE workgroup
//          scans the bucket-major (bucket, tile) table of the rows and of the edges and writes the 2 L + 1 counts, and a workgroup
//          places its tile: an element's position = the table's entry + its rank among the equal keys in front of it in the tile,
//          taken from wavefront ballots.  No position comes from an atomic.
//   fill   the placing kernels write order / new_id / hop and the renumbered node types (rows), then edge_order and the renumbered
//          edge tensors (edges, a launch later: they read new_id), then new_id[seeds].
// L + 8 launches whatever N and E; integers only; nothing synchronises, the counts travel to pinned host memory with one
// hipMemcpyAsync on the caller's stream.
#include "hgt_common.h"

namespace {

constexpr int BS = 256;                                // threads of the counting / placing workgroups
constexpr int CHUNKS = 8;                              // consecutive BS-element chunks a workgroup takes one after the other
constexpr int TILE = BS * CHUNKS;
constexpr int NBK = HGT_TRIM_MAX_LAYERS + 2;           // buckets: hop 0..L and "out"
constexpr int SCAN_BS = 1024;
constexpr int64_t LIMIT = 1ll << 31;

static inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

struct TrimLayout { uint64_t off_flag, off_hop, off_cnt_rows, off_cnt_edges, total; int64_t tiles_rows, tiles_edges; };

static TrimLayout trim_layout(int64_t N, int64_t E, int32_t L) {
    TrimLayout t;
    uint64_t o = 0;
    auto take = [&](uint64_t bytes) { uint64_t r = o; o = hgt_align_up(o + bytes, 256); return r; };
    t.tiles_rows = (N + TILE - 1) / TILE;
    t.tiles_edges = (E + TILE - 1) / TILE;
    t.off_flag = take(4);
    t.off_hop = take((uint64_t)N * 4);
    t.off_cnt_rows = take((uint64_t)t.tiles_rows * (L + 2) * 4);
    t.off_cnt_edges = take((uint64_t)t.tiles_edges * (L + 2) * 4);
    t.total = o;
    return t;
}

__global__ void k_trim_init(int32_t* __restrict__ hop, int64_t N, int32_t out_hop, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *flag = 0;
    if (i < N) hop[i] = out_hop;
}

__global__ void k_trim_seeds(const int64_t* __restrict__ seeds, int64_t S, int64_t N, int32_t* __restrict__ hop, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const int64_t v = seeds[i];
    if (v < 0 || v >= N) { atomicOr(flag, HGT_TRIM_BAD_ID); return; }
    hop[v] = 0;                                        // (every writer writes 0)
}

__global__ void k_trim_round(const int64_t* __restrict__ ei, int64_t sr, int64_t sc, int64_t E, int64_t N, int32_t r,
                             int32_t* __restrict__ hop, int32_t* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t s = ei[e * sc], t = ei[sr + e * sc];
    if (s < 0 || s >= N || t < 0 || t >= N) {
        if (r == 1) atomicOr(flag, HGT_TRIM_BAD_ID);
        return;
    }
    if (hop[t] == r - 1 && hop[s] > r) atomicMin(&hop[s], r);
}

// bucket of a row: its hop (0..L, or L + 1 = out)
struct RowKey {
    const int32_t* hop;
    __device__ __forceinline__ int operator()(int64_t i) const { return hop[i]; }
};

// bucket of an edge: its target's hop where the edge is kept (<= L - 1), else L + 1
struct EdgeKey {
    const int64_t* ei; int64_t sr, sc, N; const int32_t* hop; int32_t L;
    __device__ __forceinline__ int operator()(int64_t e) const {
        const int64_t s = ei[e * sc], t = ei[sr + e * sc];
        if (s < 0 || s >= N || t < 0 || t >= N) return L + 1;
        const int32_t h = hop[t];
        return h <= L - 1 ? h : L + 1;
    }
};

template <typename Key>
__global__ __launch_bounds__(BS) void k_trim_count(Key key, int64_t n, int64_t n_tiles, int32_t n_buckets, int32_t* __restrict__ cnt) {
    __shared__ int32_t hist[NBK];
    if (threadIdx.x < NBK) hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * TILE;
    for (int c = 0; c < CHUNKS; ++c) {
        const int64_t i = base + c * BS + threadIdx.x;
        if (i < n) atomicAdd(&hist[key(i)], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < n_buckets) cnt[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = hist[threadIdx.x];
}

// exclusive scan of a[0, n) in place by ONE workgroup of SCAN_BS threads
__device__ void scan_in_place(int32_t* __restrict__ a, int64_t n) {
    __shared__ int32_t wsum[SCAN_BS / 64];
    __shared__ int32_t carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += SCAN_BS) {
        const int64_t i = base + threadIdx.x;
        const int32_t v = i < n ? a[i] : 0;
        int32_t x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int w = 0; w < SCAN_BS / 64; ++w) {
            const int32_t s = wsum[w];
            if (w < wave) before += s;
            total += s;
        }
        const int32_t c = carry;
        if (i < n) a[i] = c + before + x - v;
        __syncthreads();
        if (threadIdx.x == 0) carry = c + total;
        __syncthreads();
    }
}

// counts: n_rows[0..L], n_edges[1..L], flag
__global__ __launch_bounds__(SCAN_BS) void k_trim_scan(int32_t* __restrict__ cnt_rows, int64_t tiles_rows, int32_t* __restrict__ cnt_edges,
                                                       int64_t tiles_edges, int32_t L, const int32_t* __restrict__ flag,
                                                       int32_t* __restrict__ counts) {
    scan_in_place(cnt_rows, tiles_rows * (L + 2));
    scan_in_place(cnt_edges, tiles_edges * (L + 2));
    __syncthreads();
    const int k = threadIdx.x;
    // the rows with hop <= L - k stand in front of bucket L - k + 1
    if (k <= L) counts[k] = tiles_rows > 0 ? cnt_rows[(int64_t)(L - k + 1) * tiles_rows] : 0;
    if (k >= 1 && k <= L) counts[L + k] = tiles_edges > 0 ? cnt_edges[(int64_t)(L - k + 1) * tiles_edges] : 0;
    if (k == 0) counts[2 * L + 1] = *flag;
}

// Stable placement of a tile: write(i, bucket, position) for every element i of the tile, position = off[bucket][tile] + the number
// of elements of the same bucket in front of i inside the tile.
template <typename Key, typename Write>
__global__ __launch_bounds__(BS) void k_trim_place(Key key, Write write, int64_t n, int64_t n_tiles, int32_t n_buckets,
                                                   const int32_t* __restrict__ off) {
    __shared__ int32_t base[NBK];
    __shared__ int32_t wcnt[BS / 64][NBK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)threadIdx.x < n_buckets) base[threadIdx.x] = off[(int64_t)threadIdx.x * n_tiles + blockIdx.x];
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * TILE;
    for (int c = 0; c < CHUNKS; ++c) {
        const int64_t i = first + c * BS + threadIdx.x;
        if (first + c * BS >= n) break;                             // (uniform over the workgroup)
        const int k = i < n ? key(i) : -1;
        int rank = 0;
        for (int b = 0; b < n_buckets; ++b) {
            const unsigned long long m = __ballot(k == b);
            if (k == b) rank = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[wave][b] = __popcll(m);
        }
        __syncthreads();
        if (k >= 0) {
            int32_t pos = base[k] + rank;
            for (int w = 0; w < wave; ++w) pos += wcnt[w][k];
            write(i, k, pos);
        }
        __syncthreads();
        if ((int)threadIdx.x < n_buckets) {
            int32_t s = 0;
            for (int w = 0; w < BS / 64; ++w) s += wcnt[w][threadIdx.x];
            base[threadIdx.x] += s;
        }
        __syncthreads();
    }
}

struct RowWrite {
    const int64_t* node_type; int32_t L;
    int32_t* hop_out; int64_t* order; int64_t* new_id; int64_t* node_type_out;
    __device__ __forceinline__ void operator()(int64_t i, int k, int32_t pos) const {
        if (k <= L) {                                   // pos < n_rows[0] <= N
            order[pos] = i;
            new_id[i] = pos;
            hop_out[i] = k;
            node_type_out[pos] = node_type[i];
        } else {
            new_id[i] = -1;
            hop_out[i] = -1;
        }
    }
};

struct EdgeWrite {
    const int64_t* ei; int64_t sr, sc; const int64_t* edge_type; const int64_t* edge_time; const int64_t* new_id; int32_t L; int64_t E;
    int64_t* edge_order; int64_t* ei_out; int64_t* edge_type_out; int64_t* edge_time_out;
    __device__ __forceinline__ void operator()(int64_t e, int k, int32_t pos) const {
        if (k > L - 1) return;                          // dropped (or an end outside [0, N): EdgeKey put it there)
        edge_order[pos] = e;                            // pos < n_edges[1] <= E
        ei_out[pos] = new_id[ei[e * sc]];
        ei_out[E + pos] = new_id[ei[sr + e * sc]];
        edge_type_out[pos] = edge_type[e];
        if (edge_time) edge_time_out[pos] = edge_time[e];
    }
};

__global__ void k_trim_out_rows(const int64_t* __restrict__ seeds, int64_t S, int64_t N, const int64_t* __restrict__ new_id,
                                int64_t* __restrict__ out_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const int64_t v = seeds[i];
    out_rows[i] = (v < 0 || v >= N) ? -1 : new_id[v];
}

static int check_sizes(int64_t N, int64_t E, int64_t S, int32_t L) {
    if (N < 0 || E < 0 || S < 0 || L < 1 || L > HGT_TRIM_MAX_LAYERS) return HGT_ERR_INVALID_ARG;
    if (N >= LIMIT || E >= LIMIT || S >= LIMIT) return HGT_ERR_INVALID_ARG;
    return HGT_OK;
}

}  // namespace

extern "C" int hgt_trim_tmp_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_layers, uint64_t* tmp_bytes_host) {
    if (!tmp_bytes_host) return HGT_ERR_INVALID_ARG;
    const int rc = check_sizes(n_nodes, n_edges, 0, n_layers);
    if (rc != HGT_OK) return rc;
    *tmp_bytes_host = trim_layout(n_nodes, n_edges, n_layers).total;
    return HGT_OK;
}

extern "C" int hgt_trim_hops(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, int64_t n_nodes, int64_t n_edges,
                             const int64_t* seeds, int64_t n_seeds, int32_t n_layers, void* tmp, uint64_t tmp_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check_sizes(n_nodes, n_edges, n_seeds, n_layers);
    if (rc != HGT_OK) return rc;
    if (!tmp || (n_edges > 0 && !edge_index) || (n_seeds > 0 && !seeds)) return HGT_ERR_INVALID_ARG;
    const TrimLayout T = trim_layout(n_nodes, n_edges, n_layers);
    if (tmp_bytes < T.total) return HGT_ERR_WORKSPACE;
    int32_t* flag = (int32_t*)((char*)tmp + T.off_flag);
    int32_t* hop = (int32_t*)((char*)tmp + T.off_hop);
    k_trim_init<<<nblk(n_nodes > 1 ? n_nodes : 1, BS), BS, 0, stream>>>(hop, n_nodes, n_layers + 1, flag);
    if (n_seeds > 0) k_trim_seeds<<<nblk(n_seeds, BS), BS, 0, stream>>>(seeds, n_seeds, n_nodes, hop, flag);
    if (n_edges > 0)
        for (int32_t r = 1; r <= n_layers; ++r)
            k_trim_round<<<nblk(n_edges, BS), BS, 0, stream>>>(edge_index, stride_row, stride_col, n_edges, n_nodes, r, hop, flag);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_trim_fill(const int64_t* edge_index, int64_t stride_row, int64_t stride_col, const int64_t* edge_type,
                             const int64_t* edge_time, const int64_t* node_type, int64_t n_nodes, int64_t n_edges, const int64_t* seeds,
                             int64_t n_seeds, int32_t n_layers, void* tmp, uint64_t tmp_bytes, int32_t* hop_out, int64_t* order,
                             int64_t* new_id, int64_t* edge_order, int64_t* node_type_out, int64_t* edge_index_out,
                             int64_t* edge_type_out, int64_t* edge_time_out, int64_t* out_rows, int32_t* counts,
                             void* counts_host_pinned, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = check_sizes(n_nodes, n_edges, n_seeds, n_layers);
    if (rc != HGT_OK) return rc;
    if (!tmp || !counts || !counts_host_pinned) return HGT_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!node_type || !hop_out || !order || !new_id || !node_type_out)) return HGT_ERR_INVALID_ARG;
    if (n_edges > 0 && (!edge_index || !edge_type || !edge_order || !edge_index_out || !edge_type_out)) return HGT_ERR_INVALID_ARG;
    if (n_edges > 0 && edge_time && !edge_time_out) return HGT_ERR_INVALID_ARG;
    if (n_seeds > 0 && (!seeds || !out_rows)) return HGT_ERR_INVALID_ARG;
    const int32_t L = n_layers;
    const TrimLayout T = trim_layout(n_nodes, n_edges, L);
    if (tmp_bytes < T.total) return HGT_ERR_WORKSPACE;
    const int32_t* flag = (const int32_t*)((char*)tmp + T.off_flag);
    const int32_t* hop = (const int32_t*)((char*)tmp + T.off_hop);
    int32_t* cnt_rows = (int32_t*)((char*)tmp + T.off_cnt_rows);
    int32_t* cnt_edges = (int32_t*)((char*)tmp + T.off_cnt_edges);
    const RowKey rk{hop};
    const EdgeKey ek{edge_index, stride_row, stride_col, n_nodes, hop, L};
    if (T.tiles_rows > 0) k_trim_count<RowKey><<<(unsigned)T.tiles_rows, BS, 0, stream>>>(rk, n_nodes, T.tiles_rows, L + 2, cnt_rows);
    if (T.tiles_edges > 0) k_trim_count<EdgeKey><<<(unsigned)T.tiles_edges, BS, 0, stream>>>(ek, n_edges, T.tiles_edges, L + 2, cnt_edges);
    k_trim_scan<<<1, SCAN_BS, 0, stream>>>(cnt_rows, T.tiles_rows, cnt_edges, T.tiles_edges, L, flag, counts);
    if (T.tiles_rows > 0) {
        const RowWrite rw{node_type, L, hop_out, order, new_id, node_type_out};
        k_trim_place<RowKey, RowWrite><<<(unsigned)T.tiles_rows, BS, 0, stream>>>(rk, rw, n_nodes, T.tiles_rows, L + 2, cnt_rows);
    }
    if (T.tiles_edges > 0) {
        const EdgeWrite ew{edge_index, stride_row, stride_col, edge_type, edge_time, new_id, L, n_edges,
                           edge_order, edge_index_out, edge_type_out, edge_time_out};
        k_trim_place<EdgeKey, EdgeWrite><<<(unsigned)T.tiles_edges, BS, 0, stream>>>(ek, ew, n_edges, T.tiles_edges, L + 2, cnt_edges);
    }
    if (n_seeds > 0) k_trim_out_rows<<<nblk(n_seeds, BS), BS, 0, stream>>>(seeds, n_seeds, n_nodes, new_id, out_rows);
    HGT_CHECK_LAUNCH();
    if (hipMemcpyAsync(counts_host_pinned, counts, (size_t)(2 * L + 2) * 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return HGT_ERR_LAUNCH;
    return HGT_OK;
}
