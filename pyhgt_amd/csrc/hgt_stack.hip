// Stacking sampled batches on the device (gfx950): B graphs that are each in hgt_plan_from_sorted form -- type-contiguous node ids,
// edges grouped by relation with non-decreasing targets -- become ONE block-diagonal graph in the same form, so that
// hgt_plan_from_sorted takes it as it stands (no radix sort) and the layer runs B batches for the launch count of one
// (pyhgt_amd/sampled.py, stack_device_graphs).
//
//   stacked node order   type, then piece, then the piece's own order
//   stacked edge order   relation, then target type, then piece, then the piece's own order: targets stay non-decreasing inside a
//                        relation, also for `self`, which has targets of every type
//   node_map / edge_map  stacked position -> position in the piece-after-piece concatenation (both are permutations)
//
// Three launches, no sort, no atomics:
//   k_stack_bounds   one thread per (piece, relation): the relation's segment of the piece and, by binary search of the piece's
//                    type_off in the segment's targets, its T sub-segments (one per target type)
//   k_stack_scan     one workgroup: exclusive sums of the B*R*T sub-segment lengths in (relation, type, piece) order and of the B*T
//                    type counts in (type, piece) order -> destination bases, rel_ptr and type_off of the stacked graph
//   k_stack_scatter  one lane per edge, then per node, of the concatenation: (piece, relation, type) by binary search of its
//                    POSITION in the tables above, rank = position - start of the sub-segment, destination = base + rank
//
// Because the rank comes from the position and the tables are forced to be a partition of [0, E_b) / [0, N_b) (k_stack_bounds
// clamps every boundary into range and keeps boundaries monotone), every position has exactly one destination inside [0, E_tot) /
// [0, N_tot) whatever the arrays hold: the maps are permutations and no store can leave its array -- it is bounds-checked all the
// same.  A piece that breaks the precondition is REPORTED through the stacked graph itself:
//   * targets not sorted inside a sub-segment: the pair stays adjacent and out of order -> hgt_plan_from_sorted sets bad_index bit 2
//   * a target whose type is not the type of its sub-segment (an unsorted pair across a type line), an id outside the piece:
//     the stacked id is written as -1 -> bad_index bit 0
//   * rel_ptr / type_off of a piece not monotone or not spanning the piece: rel_ptr_out[R] is written as -1 -> bad_index bit 2
// and the next forward raises the IndexError of GraphPlan.raise_if_bad.
#include "hgt_common.h"

namespace {

// int32 arrays inside `tmp`, a pure function of (B, T, R)
struct StackTmp {
    int64_t start;      // [B][R*T + 1]  piece-relative start of sub-segment (r, t) of piece b; entry R*T = E_b
    int64_t tb;         // [B][T + 1]    forced type boundaries of piece b (0 ... N_b)
    int64_t ebase;      // [R*T][B]      destination of the first edge of sub-segment (r, t, b)
    int64_t nbase;      // [T][B]        destination of the first node of (t, b)
    int64_t bad;        // [B][R]        1 = the piece's rel_ptr / type_off is malformed (written by every k_stack_bounds thread)
    int64_t edge_off;   // [B + 1]       the host's offsets of the pieces in the concatenation
    int64_t node_off;   // [B + 1]
    int64_t total;      // number of int32 entries
};

inline StackTmp stack_tmp(int64_t B, int64_t T, int64_t R) {
    StackTmp L;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += n; return r; };
    L.start = take(B * (R * T + 1));
    L.tb = take(B * (T + 1));
    L.ebase = take(R * T * B);
    L.nbase = take(T * B);
    L.bad = take(B * R);
    L.edge_off = take(B + 1);
    L.node_off = take(B + 1);
    L.total = o;
    return L;
}

// the pieces' offsets travel as a kernel argument: no host copy, no device allocation
struct StackOffsets {
    int32_t edge[HGT_STACK_MAX_PIECES + 1];
    int32_t node[HGT_STACK_MAX_PIECES + 1];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// first position in [lo, hi) of a[] whose value is >= key (a[] non-decreasing; on other data: some position in [lo, hi])
__device__ __forceinline__ int lower_bound_i32(const int32_t* __restrict__ a, int lo, int hi, int key) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// last index k in [0, n) with a[k] <= v, for a[0] <= v (a[] non-decreasing, n >= 1); the result is in [0, n) on any data
__device__ __forceinline__ int last_le_i32(const int32_t* __restrict__ a, int n, int v) {
    int lo = 0, hi = n;      // a[lo] <= v < a[hi] (a[n] = +inf)
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) k_stack_bounds(const int32_t* __restrict__ dst, const int32_t* __restrict__ rel_ptr,
                                                      const int32_t* __restrict__ type_off, StackOffsets off, int B, int T, int R,
                                                      int32_t* __restrict__ tmp, StackTmp L) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= B) {
        tmp[L.edge_off + i] = off.edge[i];
        tmp[L.node_off + i] = off.node[i];
    }
    if (i >= B * R) return;
    const int b = i / R, r = i - b * R;
    const int e0 = off.edge[b], Eb = off.edge[b + 1] - e0, Nb = off.node[b + 1] - off.node[b];
    const int32_t* __restrict__ rp = rel_ptr + (int64_t)b * (R + 1);
    const int32_t* __restrict__ to = type_off + (int64_t)b * (T + 1);
    int bad = 0;
    // the relation's segment [lo, hi): boundary q = clamp(max(boundary q - 1, rel_ptr[q])), boundary 0 = 0, boundary R = E_b
    int lo = 0;
    for (int q = 1; q <= r; ++q) lo = max(lo, clampi(rp[q], 0, Eb));
    const int hi = r + 1 == R ? Eb : max(lo, clampi(rp[r + 1], 0, Eb));
    if (rp[r] != lo || rp[r + 1] != hi) bad = 1;
    int32_t* __restrict__ st = tmp + L.start + (int64_t)b * (R * T + 1) + r * T;
    int32_t* __restrict__ tb = tmp + L.tb + (int64_t)b * (T + 1);
    st[0] = lo;
    if (r == 0) tb[0] = 0;
    int tprev = 0, sprev = lo;
    for (int t = 1; t < T; ++t) {
        const int tcur = clampi(max(tprev, to[t]), 0, Nb);
        if (to[t] != tcur) bad = 1;
        sprev = lower_bound_i32(dst + e0, sprev, hi, tcur);      // searched from the previous boundary on: monotone on any data
        st[t] = sprev;
        if (r == 0) tb[t] = tcur;
        tprev = tcur;
    }
    if (to[0] != 0 || to[T] != Nb) bad = 1;
    if (r == 0) tb[T] = Nb;
    if (r == R - 1) st[T] = Eb;
    tmp[L.bad + i] = bad;
}

constexpr int SCAN_THREADS = 1024;

// exclusive sums of n counts (count(i) >= 0) over one workgroup: thread k owns the chunk [k * chunk, (k + 1) * chunk)
template <class Count, class Emit>
__device__ __forceinline__ void block_exclusive_scan(int n, int32_t* sh, Count count, Emit emit) {
    const int k = threadIdx.x;
    const int chunk = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const int beg = min(n, k * chunk), end = min(n, beg + chunk);
    int sum = 0;
    for (int i = beg; i < end; ++i) sum += count(i);
    __syncthreads();      // sh[] may still be read by the previous scan
    sh[k] = sum;
    __syncthreads();
    for (int step = 1; step < SCAN_THREADS; step <<= 1) {
        const int add = k >= step ? sh[k - step] : 0;
        __syncthreads();
        sh[k] += add;
        __syncthreads();
    }
    int run = sh[k] - sum;
    for (int i = beg; i < end; ++i) {
        emit(i, run);
        run += count(i);
    }
}

__global__ void __launch_bounds__(SCAN_THREADS) k_stack_scan(int B, int T, int R, int E_tot, int N_tot, int32_t* __restrict__ tmp, StackTmp L,
                                                             int32_t* __restrict__ rel_ptr_out, int32_t* __restrict__ type_off_out) {
    __shared__ int32_t sh[SCAN_THREADS];
    const int RT = R * T;
    int bad = 0;
    for (int i = threadIdx.x; i < B * R; i += SCAN_THREADS) bad |= tmp[L.bad + i];
    bad = __syncthreads_or(bad);
    const int32_t* __restrict__ start = tmp + L.start;
    const int32_t* __restrict__ tb = tmp + L.tb;
    // edges: i = (r * T + t) * B + b
    block_exclusive_scan(
        RT * B, sh,
        [&](int i) {
            const int k = i / B, b = i - k * B;
            const int32_t* s = start + (int64_t)b * (RT + 1) + k;
            return s[1] - s[0];
        },
        [&](int i, int base) {
            tmp[L.ebase + i] = base;
            if (i % (T * B) == 0) rel_ptr_out[i / (T * B)] = base;
        });
    // nodes: i = t * B + b
    block_exclusive_scan(
        T * B, sh,
        [&](int i) {
            const int t = i / B, b = i - t * B;
            const int32_t* s = tb + (int64_t)b * (T + 1) + t;
            return s[1] - s[0];
        },
        [&](int i, int base) {
            tmp[L.nbase + i] = base;
            if (i % B == 0) type_off_out[i / B] = base;
        });
    if (threadIdx.x == 0) {
        rel_ptr_out[R] = bad ? -1 : E_tot;      // -1: hgt_plan_from_sorted reports "rel_ptr does not span [0, E]"
        type_off_out[T] = N_tot;
    }
}

// stacked id of node `v` of piece b (-1: v is not a node of the piece); *type = its type
__device__ __forceinline__ int stack_node(const int32_t* __restrict__ tb, const int32_t* __restrict__ nbase, int B, int T, int b, int Nb, int v,
                                          int* type) {
    *type = -1;
    if (v < 0 || v >= Nb) return -1;
    const int t = last_le_i32(tb, T, v);      // tb[0] = 0 <= v < N_b = tb[T]: the last type that starts at or before v holds it
    *type = t;
    return nbase[t * B + b] + (v - tb[t]);
}

__global__ void __launch_bounds__(256) k_stack_scatter(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                       const int32_t* __restrict__ edge_time, int B, int T, int R, int E_tot, int N_tot,
                                                       const int32_t* __restrict__ tmp, StackTmp L, int32_t* __restrict__ src_out,
                                                       int32_t* __restrict__ dst_out, int32_t* __restrict__ edge_time_out,
                                                       int32_t* __restrict__ node_map, int32_t* __restrict__ edge_map) {
    const int RT = R * T;
    const int32_t* __restrict__ edge_off = tmp + L.edge_off;
    const int32_t* __restrict__ node_off = tmp + L.node_off;
    const int32_t* __restrict__ nbase = tmp + L.nbase;
    const int64_t total = (int64_t)E_tot + N_tot, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g64 < total; g64 += stride) {
        if (g64 < E_tot) {
            const int g = (int)g64;
            const int b = last_le_i32(edge_off, B, g);      // the last piece that starts at or before g: never an empty one
            const int e = g - edge_off[b];
            const int32_t* __restrict__ start = tmp + L.start + (int64_t)b * (RT + 1);
            const int k = last_le_i32(start, RT, e);        // sub-segment (r, t) = (k / T, k % T)
            const int p = tmp[L.ebase + (int64_t)k * B + b] + (e - start[k]);
            if (e < 0 || p < 0 || p >= E_tot) continue;     // cannot happen: the tables are a partition (see the head of the file)
            const int32_t* __restrict__ tb = tmp + L.tb + (int64_t)b * (T + 1);
            const int Nb = node_off[b + 1] - node_off[b];
            int ts, td;
            const int s = stack_node(tb, nbase, B, T, b, Nb, src[g], &ts);
            int d = stack_node(tb, nbase, B, T, b, Nb, dst[g], &td);
            if (td != k % T) d = -1;                        // target of another type than its sub-segment: the piece is not sorted
            src_out[p] = s;
            dst_out[p] = d;
            if (edge_time_out) edge_time_out[p] = edge_time[g];
            edge_map[p] = g;
        } else {
            const int g = (int)(g64 - E_tot);
            const int b = last_le_i32(node_off, B, g);
            const int v = g - node_off[b];
            const int32_t* __restrict__ tb = tmp + L.tb + (int64_t)b * (T + 1);
            int t;
            const int p = stack_node(tb, nbase, B, T, b, node_off[b + 1] - node_off[b], v, &t);
            if (p < 0 || p >= N_tot) continue;              // cannot happen
            node_map[p] = g;
        }
    }
}

constexpr int64_t STACK_MAX_BLOCKS = 8192;
constexpr int64_t STACK_MAX_SEGMENTS = (int64_t)1 << 22;      // B * R * T: what one workgroup scans in a few chunks per thread

}  // namespace

extern "C" int hgt_stack_tmp_bytes(int32_t n_pieces, int32_t n_types, int32_t n_relations, uint64_t* bytes_host) {
    if (!bytes_host || n_pieces < 1 || n_types < 1 || n_relations < 1) return HGT_ERR_INVALID_ARG;
    if (n_pieces > HGT_STACK_MAX_PIECES) return HGT_ERR_UNSUPPORTED;
    if ((int64_t)n_pieces * n_types * n_relations > STACK_MAX_SEGMENTS) return HGT_ERR_TOO_LARGE;
    *bytes_host = (uint64_t)stack_tmp(n_pieces, n_types, n_relations).total * 4;
    return HGT_OK;
}

extern "C" int hgt_stack_sorted(const int32_t* src, const int32_t* dst, const int32_t* edge_time, const int32_t* rel_ptr,
                                const int32_t* type_off, const int64_t* edge_off_host, const int64_t* node_off_host, int32_t n_pieces,
                                int32_t n_types, int32_t n_relations, int32_t* src_out, int32_t* dst_out, int32_t* edge_time_out,
                                int32_t* rel_ptr_out, int32_t* type_off_out, int32_t* node_map, int32_t* edge_map, void* tmp,
                                uint64_t tmp_bytes, void* stream) {
    const int B = n_pieces, T = n_types, R = n_relations;
    if (B < 1 || T < 1 || R < 1 || !rel_ptr || !type_off || !edge_off_host || !node_off_host || !rel_ptr_out || !type_off_out || !tmp)
        return HGT_ERR_INVALID_ARG;
    if (B > HGT_STACK_MAX_PIECES) return HGT_ERR_UNSUPPORTED;
    if ((int64_t)B * T * R > STACK_MAX_SEGMENTS) return HGT_ERR_TOO_LARGE;
    if (edge_off_host[0] != 0 || node_off_host[0] != 0) return HGT_ERR_INVALID_ARG;
    for (int b = 0; b < B; ++b)
        if (edge_off_host[b + 1] < edge_off_host[b] || node_off_host[b + 1] < node_off_host[b]) return HGT_ERR_INVALID_ARG;
    const int64_t E_tot = edge_off_host[B], N_tot = node_off_host[B];
    if (E_tot > 0x7fffffff || N_tot > 0x7fffffff) return HGT_ERR_TOO_LARGE;
    if (E_tot > 0 && (!src || !dst || !src_out || !dst_out || !edge_map)) return HGT_ERR_INVALID_ARG;
    if (N_tot > 0 && !node_map) return HGT_ERR_INVALID_ARG;
    if ((edge_time == nullptr) != (edge_time_out == nullptr)) return HGT_ERR_INVALID_ARG;
    const StackTmp L = stack_tmp(B, T, R);
    if (tmp_bytes < (uint64_t)L.total * 4) return HGT_ERR_WORKSPACE;
    StackOffsets off;
    for (int b = 0; b <= HGT_STACK_MAX_PIECES; ++b) {
        off.edge[b] = (int32_t)edge_off_host[b < B ? b : B];
        off.node[b] = (int32_t)node_off_host[b < B ? b : B];
    }
    hipStream_t st = (hipStream_t)stream;
    int32_t* t32 = (int32_t*)tmp;
    k_stack_bounds<<<(unsigned)((B * R + 256) / 256), 256, 0, st>>>(dst, rel_ptr, type_off, off, B, T, R, t32, L);
    HGT_CHECK_LAUNCH();
    k_stack_scan<<<1, SCAN_THREADS, 0, st>>>(B, T, R, (int)E_tot, (int)N_tot, t32, L, rel_ptr_out, type_off_out);
    HGT_CHECK_LAUNCH();
    const int64_t total = E_tot + N_tot;
    if (total > 0) {
        const int64_t blocks = (total + 255) / 256;
        k_stack_scatter<<<(unsigned)(blocks < STACK_MAX_BLOCKS ? blocks : STACK_MAX_BLOCKS), 256, 0, st>>>(
            src, dst, edge_time, B, T, R, (int)E_tot, (int)N_tot, t32, L, src_out, dst_out, edge_time_out, node_map, edge_map);
        HGT_CHECK_LAUNCH();
    }
    return HGT_OK;
}
