// HGSampling on the device (gfx950): the budget sampler of pyHGT/data.py:87-210 over a graph that lives in device memory, so that a
// training loop gets its sampled sub-graphs -- already in the sorted int32 form of hgt_plan_from_sorted / hgt_stack_sorted -- without
// a host copy of an index (pyhgt_amd/sampler.py).
//
// Resident graph     per meta triple (target type, source type, relation): a CSR by target id -- indptr int32[n_tgt + 1], src int32[],
//                    time int32[] (HGT_SAMPLER_TIME_NONE = the reference's None: the neighbour inherits the target's time, data.py:125)
// State per type     score u64[n] (32.32 fixed point), stamp u64[n] ((step << 32) | (time ^ 0x80000000)), serial int32[n] (-1 = not
//                    sampled), the list of sampled ids in serial order, the list of candidates (budget keys), counts[4] = {number
//                    sampled, first serial of the newest batch, number of candidates, overflow flag}
// Random words       Philox4x32-10 (hgt_philox.h), key = seed, word 0 of the counter
//                      neighbour subset  (position in the row, target id, step, 0x10000 + triple index)
//                      selection         (node id, type, step, 0x20000)
//                    -- a function of what is drawn, never of the launch geometry.
//
//   hgt_sampler_seed        serial / stamp / sampled list of the seed nodes of one type
//   hgt_sampler_add_budget  data.py:112-130 for the newest batch of one type over every triple into it.  One wavefront per
//                           (node, triple) row up to HGT_SAMPLER_HUB_DEG = 512 neighbours (8 per lane, their Philox words in
//                           registers); longer rows (venues, fields) are queued and each taken by a 1024-thread workgroup in a second
//                           launch (first 8192 words in registers, the rest recomputed per pass).  A row with more than
//                           sampled_number neighbours keeps the sampled_number smallest (word, position): the threshold word by
//                           bisection on counts (32 passes over the row), ties on the word by bisection on the position.  Survivors:
//                           u64 atomicAdd of round(2^32 / len) into score, u64 atomicMax into stamp, first touch appends to the
//                           candidate list.  Integer atomics only: the state is bit-reproducible whatever the order.
//   hgt_sampler_select      data.py:151-172 for one type: key = -log(u) / s^2 in fp32 (Efraimidis-Spirakis), u = ((word >> 8) + 0.5)
//                           * 2^-24, the min(sampled_number, candidates) smallest (key, node id) chosen and given serials in that
//                           order.  u above 1/2 is not a fp32 number ((word >> 8) + 0.5 needs 25 bits there), so for those words
//                           -log(u) is taken as -log1pf(-(1 - u)) with 1 - u exact: the key is that of the exact u either way.
//                           One launch for the keys, one 1024-thread workgroup for threshold (64-bit bisection), compaction of the
//                           candidates that stay, and ranks.
//   hgt_sampler_induce_count / _fill   data.py:183-209 + 240-250: per (triple, sampled target) row the neighbours that are sampled,
//                           counted, scanned (one workgroup), then written relation-major in global target order with
//                           edge_time = time[tgt] - time[src] + 120; `self` edges last.  Rows above the hub line take a workgroup,
//                           as in add_budget.  The caller reads sizes_out between the two calls (the only host read of a batch).
//   hgt_sampler_induce_count_masked / _fill_masked   the same two passes with a pair of thresholds per triple (task batches: the label
//                           edges at the seeds, OAG/train_paper_field.py:109-122): an edge between the target of serial i and a source
//                           of serial ser is left out iff i < tgt_below or ser < src_below.  The thresholds ride next to the tables
//                           as a kernel argument; the unmasked entry points run the same kernels with all-zero thresholds.
//   hgt_sampler_reset       walks the sampled and candidate lists and clears exactly the entries the call touched
//   hgt_sampler_*_batched   the same steps for n_batch independent batches (replicas) at once: replica b of every launch is blockIdx.y = b,
//                           its state the table's pointers shifted by b strides (View), its Philox key one of n_batch pairs in the
//                           argument space.  The row logic below exists once; the single entry points keep their own instantiations.
//   hgt_sampler_gather_features   the feature rows of a batched call in one launch, one wavefront per output row
// No float atomics in this file; compiled without fast-math like the rest of the library.
#include "hgt_graph_rule.h"
#include "hgt_philox.h"

namespace {

constexpr int HUB = HGT_SAMPLER_HUB_DEG;      // 8 neighbours per lane of a wavefront
constexpr int WREG = 8;                       // Philox words a lane keeps in registers
constexpr int BIG = 1024;                     // threads of the single-workgroup kernels and of the hub kernels
static_assert(HUB == WREG * HGT_WAVE, "the hub line is what one wavefront holds in registers");

// every table of a call travels as a kernel argument: no device allocation, no host copy
struct Tables {
    hgt_sampler_type ty[HGT_SAMPLER_MAX_TYPES];
    hgt_sampler_triple tr[HGT_SAMPLER_MAX_TRIPLES];
    int32_t slot_off[HGT_SAMPLER_MAX_TRIPLES + 1];      // induce: first row slot of triple m (slots of m: cap_sampled of its target type)
    int32_t T, M;
};

// induce: one pair of thresholds per triple, next to the tables in the kernel-argument space (all zero: nothing is masked)
struct Masks {
    hgt_sampler_mask m[HGT_SAMPLER_MAX_TRIPLES];
};
// a launch carries 4 KB of arguments: the tables, the thresholds and the scalars and pointers of the induce kernels (below 128 bytes)
static_assert(sizeof(Tables) + sizeof(Masks) + 128 <= 4096, "the argument structs of the induce kernels do not fit one launch");

struct BudgetParams {
    int32_t t, step, sn, has_max, max_time, max_new, ntr;
    uint32_t k0, k1;
    uint8_t sel[HGT_SAMPLER_MAX_TRIPLES];      // the triples into type t
};

__device__ __forceinline__ uint32_t time_bias(int32_t t) { return (uint32_t)t ^ 0x80000000u; }
__device__ __forceinline__ int32_t stamp_time(uint64_t s) { return (int32_t)((uint32_t)s ^ 0x80000000u); }
__device__ __forceinline__ int clamp0(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// sum of c over the group: a wavefront (G = 64) or the whole workgroup (G = BIG; every thread must call, sh = 16 ints of LDS)
template <int G>
__device__ __forceinline__ int group_sum(int c, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if constexpr (G == HGT_WAVE) return c;
    const int wave = threadIdx.x >> 6;
    __syncthreads();      // sh[] may still be read by the previous call
    if ((threadIdx.x & 63) == 0) sh[wave] = c;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < G / HGT_WAVE; ++w) total += sh[w];
    return total;
}

// exclusive prefix of a 0/1 flag over the group in lane order, *total = the group's sum
template <int G>
__device__ __forceinline__ int group_scan_flag(bool flag, int* total, int* sh) {
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63;
    int prefix = __popcll(b & ((1ull << lane) - 1ull));
    const int mine = __popcll(b);
    if constexpr (G == HGT_WAVE) {
        *total = mine;
        return prefix;
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wave] = mine;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < G / HGT_WAVE; ++w) {
        if (w < wave) prefix += sh[w];
        tot += sh[w];
    }
    *total = tot;
    return prefix;
}

// ------------------------------------------------------------------------------------------------ replica view
// A batched call (hgt_sampler_*_batched) runs n_batch independent batches in one pass of launches, replica b = blockIdx.y.  The tables
// stay those of one replica; View hands the row logic below the state of a type as replica b sees it: the table's pointers shifted by b
// strides (n_nodes, cap_sampled, cap_cand, 4 * T -- fields of the tables themselves), one 64-byte entry on demand.  BATCHED = false is
// the table's entry as it is: the kernels of the single entry points are their own instantiations, without a replica index or a stride.
template <bool BATCHED>
struct View {
    const Tables& tb;
    int b;
    __device__ __forceinline__ hgt_sampler_type ty(int t) const {
        hgt_sampler_type S = tb.ty[t];
        if constexpr (BATCHED) {
            S.score += (int64_t)b * S.n_nodes;
            S.stamp += (int64_t)b * S.n_nodes;
            S.serial += (int64_t)b * S.n_nodes;
            S.sampled += (int64_t)b * S.cap_sampled;
            S.cand += (int64_t)b * S.cap_cand;
            S.counts += (int64_t)b * 4 * tb.T;
        }
        return S;
    }
};

// the Philox keys of the replicas, in the kernel-argument space next to the tables
struct Keys {
    uint32_t k[HGT_SAMPLER_MAX_BATCH][2];
};
// this is what bounds HGT_SAMPLER_MAX_BATCH: tables + budget parameters + keys + the pointers and scalars of k_budget_batched (below
// 128 bytes) inside the 4 KB of arguments of a launch
static_assert(sizeof(Tables) + sizeof(BudgetParams) + sizeof(Keys) + 128 <= 4096, "the keys of HGT_SAMPLER_MAX_BATCH replicas do not fit one launch");
static_assert(HGT_SAMPLER_MAX_BATCH >= 16, "a training step stacks 16 pieces");

// fill pass of a batched call: where replica b's piece lies in the concatenated outputs.  offs = node prefix sums [B + 1], then edge
// prefix sums [B + 1] (k_batch_offsets); false: the range is not inside the totals the host allocated, the replica writes nothing
struct Range {
    int n0, nn, e0, ne;
};
__device__ __forceinline__ bool replica_range(const int32_t* __restrict__ offs, int b, int B, int n_nodes, int n_edges, Range* r) {
    const int n0 = offs[b], n1 = offs[b + 1], e0 = offs[B + 1 + b], e1 = offs[B + 2 + b];
    if (n0 < 0 || n1 < n0 || n1 > n_nodes || e0 < 0 || e1 < e0 || e1 > n_edges || e1 - e0 < n1 - n0) return false;
    *r = Range{n0, n1 - n0, e0, e1 - e0};
    return true;
}

// ------------------------------------------------------------------------------------------------ seeds
template <bool BATCHED>
__device__ __forceinline__ void seed_nodes(const View<BATCHED>& V, int t, const int32_t* __restrict__ ids, const int32_t* __restrict__ times, int n,
                                           int step) {
    const hgt_sampler_type S = V.ty(t);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        S.counts[0] = n;
        S.counts[1] = 0;
    }
    if (i >= n) return;
    const int v = ids[i];
    S.sampled[i] = v;
    if ((unsigned)v >= (unsigned)S.n_nodes) {
        S.counts[3] = 1;
        return;
    }
    S.serial[v] = i;
    S.stamp[v] = ((uint64_t)(uint32_t)step << 32) | time_bias(times[i]);
}

__global__ void __launch_bounds__(256) k_seed(Tables tb, int t, const int32_t* __restrict__ ids, const int32_t* __restrict__ times, int n,
                                               int step) {
    seed_nodes(View<false>{tb, 0}, t, ids, times, n, step);
}

__global__ void __launch_bounds__(256) k_seed_batched(Tables tb, int t, const int32_t* __restrict__ ids, const int32_t* __restrict__ times, int n,
                                                       int step) {
    const int b = blockIdx.y;
    seed_nodes(View<true>{tb, b}, t, ids + (int64_t)b * n, times + (int64_t)b * n, n, step);
}

// ------------------------------------------------------------------------------------------------ add_budget
// One row: target v of triple m.  `lane` in [0, G) is the thread's place in the group that owns the row.
template <int G, bool BATCHED>
__device__ __forceinline__ void budget_row(const View<BATCHED>& V, const BudgetParams& P, uint32_t k0, uint32_t k1, int m, int v, int32_t v_time,
                                           int lane, int* sh) {
    const hgt_sampler_triple& tr = V.tb.tr[m];
    const hgt_sampler_type S = V.ty(tr.src_type);
    const int beg = tr.indptr[v], deg = tr.indptr[v + 1] - beg;
    if (deg <= 0) return;
    const int sn = P.sn;
    const int len = deg < sn ? deg : sn;                                          // len(sampled_ids), data.py:119-122
    const uint64_t add = (((uint64_t)1 << 33) + (uint64_t)len) / (2ull * (uint64_t)len);      // round(2^32 / len)
    const bool choose = deg > sn;                                                 // deg == sn: choice() returns all of them
    auto word = [&](int p) { return philox4x32_10((uint32_t)p, (uint32_t)v, (uint32_t)P.step, 0x10000u + (uint32_t)m, k0, k1).w[0]; };
    uint32_t w[WREG];
    uint32_t w_star = 0xffffffffu;
    int p_star = deg;
    if (choose) {
#pragma unroll
        for (int j = 0; j < WREG; ++j) {
            const int p = lane + j * G;
            w[j] = p < deg ? word(p) : 0u;
        }
        auto count = [&](auto pred) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < WREG; ++j) {
                const int p = lane + j * G;
                if (p < deg && pred(w[j], p)) ++c;
            }
            for (int p = lane + WREG * G; p < deg; p += G)
                if (pred(word(p), p)) ++c;
            return group_sum<G>(c, sh);
        };
        // the smallest word W with #{word <= W} >= sn
        uint64_t lo = 0, hi = 0xffffffffull;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (count([&](uint32_t x, int) { return (uint64_t)x <= mid; }) >= sn) hi = mid;
            else lo = mid + 1;
        }
        w_star = (uint32_t)lo;
        const int below = count([&](uint32_t x, int) { return x < w_star; });
        const int need = sn - below;                                              // >= 1 of the words equal to W, by position
        if (count([&](uint32_t x, int) { return x == w_star; }) > need) {
            int plo = 0, phi = deg - 1;
            while (plo < phi) {
                const int mid = plo + ((phi - plo) >> 1);
                if (count([&](uint32_t x, int p) { return x == w_star && p <= mid; }) >= need) phi = mid;
                else plo = mid + 1;
            }
            p_star = plo;
        }
    }
    auto touch = [&](int p, uint32_t x) {
        if (choose && !(x < w_star || (x == w_star && p <= p_star))) return;
        const int s = tr.src[beg + p];
        if ((unsigned)s >= (unsigned)S.n_nodes) return;
        int32_t tm = tr.time[beg + p];
        if (tm == HGT_SAMPLER_TIME_NONE) tm = v_time;                            // data.py:125-126
        if (P.has_max && tm > P.max_time) return;                                 // data.py:127
        if (S.serial[s] >= 0) return;                                             // already sampled
        const unsigned long long old = atomicAdd((unsigned long long*)&S.score[s], (unsigned long long)add);
        atomicMax((unsigned long long*)&S.stamp[s], ((unsigned long long)(uint32_t)P.step << 32) | time_bias(tm));
        if (old == 0ull) {                                                        // first touch: add >= 1, so a touched score is never 0
            const int idx = atomicAdd(&S.counts[2], 1);
            if (idx < S.cap_cand) S.cand[idx] = s;
            else S.counts[3] = 1;
        }
    };
#pragma unroll
    for (int j = 0; j < WREG; ++j) {
        const int p = lane + j * G;
        if (p < deg) touch(p, choose ? w[j] : 0u);
    }
    for (int p = lane + WREG * G; p < deg; p += G) touch(p, choose ? word(p) : 0u);
}

// row `gw` of the call -> (triple, target); false: no such row
template <bool BATCHED>
__device__ __forceinline__ bool budget_decode(const View<BATCHED>& V, const BudgetParams& P, int gw, int* m, int* v, int32_t* v_time, int* deg) {
    const hgt_sampler_type Tt = V.ty(P.t);
    const int ns = clamp0(Tt.counts[0], Tt.cap_sampled), nb = clamp0(Tt.counts[1], ns);
    const int n_new = min(ns - nb, P.max_new);
    const int i = gw / P.ntr, j = gw - i * P.ntr;
    if (i >= n_new) return false;
    *m = P.sel[j];
    *v = Tt.sampled[nb + i];
    if ((unsigned)*v >= (unsigned)Tt.n_nodes) return false;
    *v_time = stamp_time(Tt.stamp[*v]);
    const int32_t* ip = V.tb.tr[*m].indptr;
    *deg = ip[*v + 1] - ip[*v];
    return true;
}

// the wavefront rows of a launch; a row above the hub line goes into the queue (*hub_n entries of hub_rows[])
template <bool BATCHED>
__device__ __forceinline__ void budget_rows(const View<BATCHED>& V, const BudgetParams& P, uint32_t k0, uint32_t k1, int32_t* __restrict__ hub_n,
                                            int32_t* __restrict__ hub_rows, int max_rows) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    int m, v, deg;
    int32_t v_time;
    if (gw >= max_rows || !budget_decode(V, P, gw, &m, &v, &v_time, &deg)) return;
    if (deg > HUB) {
        if (lane == 0) {
            const int idx = atomicAdd(hub_n, 1);
            if (idx < max_rows) hub_rows[idx] = gw;
        }
        return;
    }
    budget_row<HGT_WAVE>(V, P, k0, k1, m, v, v_time, lane, nullptr);
}

template <bool BATCHED>
__device__ __forceinline__ void budget_hub_rows(const View<BATCHED>& V, const BudgetParams& P, uint32_t k0, uint32_t k1,
                                                const int32_t* __restrict__ hub_n, const int32_t* __restrict__ hub_rows, int max_rows) {
    __shared__ int sh[BIG / HGT_WAVE];
    const int n = clamp0(*hub_n, max_rows);
    for (int h = blockIdx.x; h < n; h += gridDim.x) {
        int m, v, deg;
        int32_t v_time;
        if (!budget_decode(V, P, hub_rows[h], &m, &v, &v_time, &deg)) continue;      // workgroup-uniform
        budget_row<BIG>(V, P, k0, k1, m, v, v_time, threadIdx.x, sh);
    }
}

__global__ void __launch_bounds__(256) k_budget(Tables tb, BudgetParams P, int32_t* __restrict__ hub, int max_rows) {
    budget_rows(View<false>{tb, 0}, P, P.k0, P.k1, hub, hub + 1, max_rows);
}

__global__ void __launch_bounds__(BIG) k_budget_hub(Tables tb, BudgetParams P, const int32_t* __restrict__ hub, int max_rows) {
    budget_hub_rows(View<false>{tb, 0}, P, P.k0, P.k1, hub, hub + 1, max_rows);
}

// hub of a batched call: the B counters, then hub_stride >= max_rows entries per replica
__global__ void __launch_bounds__(256) k_budget_batched(Tables tb, BudgetParams P, Keys keys, int32_t* __restrict__ hub, int64_t hub_stride,
                                                        int max_rows) {
    const int b = blockIdx.y;
    budget_rows(View<true>{tb, b}, P, keys.k[b][0], keys.k[b][1], hub + b, hub + gridDim.y + b * hub_stride, max_rows);
}

__global__ void __launch_bounds__(BIG) k_budget_hub_batched(Tables tb, BudgetParams P, Keys keys, const int32_t* __restrict__ hub, int64_t hub_stride,
                                                            int max_rows) {
    const int b = blockIdx.y;
    budget_hub_rows(View<true>{tb, b}, P, keys.k[b][0], keys.k[b][1], hub + b, hub + gridDim.y + b * hub_stride, max_rows);
}

// ------------------------------------------------------------------------------------------------ select
template <bool BATCHED>
__device__ __forceinline__ void select_keys(const View<BATCHED>& V, int t, int step, uint32_t k0, uint32_t k1, uint64_t* __restrict__ keys) {
    const hgt_sampler_type S = V.ty(t);
    const int n = clamp0(S.counts[2], S.cap_cand);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = S.cand[i];
    const float s = (float)S.score[v] * 2.3283064365386963e-10f;                  // score * 2^-32
    const uint32_t word = philox4x32_10((uint32_t)v, (uint32_t)t, (uint32_t)step, 0x20000u, k0, k1).w[0];
    const uint32_t q = word >> 8;                                                 // u = (q + 0.5) * 2^-24
    float nlog;
    if (q < (1u << 23)) nlog = -logf(((float)q + 0.5f) * 5.9604644775390625e-8f);             // u exact in fp32
    else nlog = -log1pf(-(((float)((1u << 24) - 1u - q) + 0.5f) * 5.9604644775390625e-8f));   // 1 - u exact in fp32
    const float key = nlog / (s * s);
    keys[i] = ((uint64_t)__float_as_uint(key) << 32) | (uint32_t)v;               // key > 0: its bits order like the float
}

template <bool BATCHED>
__device__ __forceinline__ void select_pick(const View<BATCHED>& V, int t, int sn, const uint64_t* __restrict__ keys, int32_t* __restrict__ tmp) {
    __shared__ int sh[BIG / HGT_WAVE];
    __shared__ uint64_t chosen[HGT_SAMPLER_MAX_NUMBER];
    __shared__ int n_chosen, n_rest;
    const hgt_sampler_type S = V.ty(t);
    const int lane = threadIdx.x;
    const int n = clamp0(S.counts[2], S.cap_cand);
    const int base = clamp0(S.counts[0], S.cap_sampled);
    const int count = min(min(sn, n), S.cap_sampled - base);
    if (lane == 0) n_chosen = n_rest = 0;
    uint64_t k_star = ~0ull;
    if (count < n) {
        uint64_t lo = 0, hi = ~0ull;
        while (lo < hi) {                                                         // the smallest K with #{key <= K} >= count
            const uint64_t mid = lo + ((hi - lo) >> 1);
            int c = 0;
            for (int p = lane; p < n; p += BIG)                                   // 64 passes over keys[] (L2-resident)
                if (keys[p] <= mid) ++c;
            if (group_sum<BIG>(c, sh) >= count) hi = mid;
            else lo = mid + 1;
        }
        k_star = count > 0 ? lo : 0ull;
    }
    __syncthreads();
    for (int p = lane; p < n; p += BIG) {
        const uint64_t k = keys[p];
        if (count > 0 && k <= k_star) {
            const int j = atomicAdd(&n_chosen, 1);
            if (j < HGT_SAMPLER_MAX_NUMBER) chosen[j] = k;
        } else {
            tmp[atomicAdd(&n_rest, 1)] = (int32_t)(uint32_t)k;                    // n_rest <= n <= cap_cand entries of tmp
        }
    }
    __syncthreads();
    const int rest = n_rest, got = min(n_chosen, count);                          // keys are distinct (node id in the low word): got == count
    for (int p = lane; p < rest; p += BIG) S.cand[p] = tmp[p];                    // the order of the rest does not enter any result
    for (int i = lane; i < got; i += BIG) {
        const uint64_t k = chosen[i];
        int r = 0;
        for (int j = 0; j < got; ++j) r += chosen[j] < k;
        const int v = (int32_t)(uint32_t)k;
        S.sampled[base + r] = v;                                                  // base + r < base + count <= cap_sampled
        S.serial[v] = base + r;                                                   // v came out of cand[]: inside [0, n_nodes)
    }
    __syncthreads();
    if (lane == 0) {
        S.counts[1] = base;
        S.counts[0] = base + got;
        S.counts[2] = rest;
    }
}

__global__ void __launch_bounds__(256) k_select_keys(Tables tb, int t, int step, uint32_t k0, uint32_t k1, uint64_t* __restrict__ keys) {
    select_keys(View<false>{tb, 0}, t, step, k0, k1, keys);
}

__global__ void __launch_bounds__(BIG) k_select_pick(Tables tb, int t, int sn, const uint64_t* __restrict__ keys, int32_t* __restrict__ tmp) {
    select_pick(View<false>{tb, 0}, t, sn, keys, tmp);
}

// keys / tmp of a batched call: `stride` entries per replica
__global__ void __launch_bounds__(256) k_select_keys_batched(Tables tb, int t, int step, Keys seeds, uint64_t* __restrict__ keys, int64_t stride) {
    const int b = blockIdx.y;
    select_keys(View<true>{tb, b}, t, step, seeds.k[b][0], seeds.k[b][1], keys + b * stride);
}

__global__ void __launch_bounds__(BIG) k_select_pick_batched(Tables tb, int t, int sn, const uint64_t* __restrict__ keys, int32_t* __restrict__ tmp,
                                                             int64_t stride) {
    const int b = blockIdx.y;
    select_pick(View<true>{tb, b}, t, sn, keys + b * stride, tmp + b * stride);
}

// ------------------------------------------------------------------------------------------------ induce
// row slot -> (triple m, serial i of the target); deg < 0: no such row
template <bool BATCHED>
__device__ __forceinline__ void induce_decode(const View<BATCHED>& V, int slot, int* m, int* i, int* v, int* deg) {
    const Tables& tb = V.tb;
    int mm = 0;
    while (mm + 1 < tb.M && tb.slot_off[mm + 1] <= slot) ++mm;
    const hgt_sampler_type Tt = V.ty(tb.tr[mm].tgt_type);
    *m = mm;
    *i = slot - tb.slot_off[mm];
    *deg = -1;
    if (*i >= clamp0(Tt.counts[0], Tt.cap_sampled)) return;
    *v = Tt.sampled[*i];
    if ((unsigned)*v >= (unsigned)Tt.n_nodes) return;
    const int32_t* ip = tb.tr[mm].indptr;
    *deg = ip[*v + 1] - ip[*v];
}

// what the induce kernels of one replica read and write: the scratch of the two passes (hub queue = *hub_n entries of hub_rows[]), the
// replica's type_off and its piece of the outputs (n_edges = its non-self edges)
struct InduceIO {
    int32_t* rowoff;
    int32_t* hub_n;
    int32_t* hub_rows;
    const int32_t* type_off;
    int32_t* src_out;
    int32_t* dst_out;
    int32_t* time_out;
    int n_edges;
};

// FILL = false: the number of sampled neighbours of the row -> rowoff[slot];  FILL = true: the edges, from position rowoff[slot] on.
// The mask of the triple leaves out the whole row of a target with serial i < tgt_below and every source with serial < src_below; both
// passes apply it, so the offsets of the count pass are those of the edges the fill pass writes.
template <int G, bool FILL, bool BATCHED>
__device__ __forceinline__ void induce_row(const View<BATCHED>& V, const hgt_sampler_mask mk, int m, int i, int v, int deg, int slot, int lane,
                                           int* sh, const InduceIO& io) {
    const hgt_sampler_triple& tr = V.tb.tr[m];
    const hgt_sampler_type S = V.ty(tr.src_type);
    if (i < mk.tgt_below) {                                                       // uniform over the group that owns the row
        if constexpr (!FILL)
            if (lane == 0) io.rowoff[slot] = 0;
        return;
    }
    const int beg = tr.indptr[v];
    int run = 0;
    int base = 0, tgt = 0, s_off = 0;
    int32_t v_time = 0;
    if constexpr (FILL) {
        base = io.rowoff[slot];
        tgt = io.type_off[tr.tgt_type] + i;
        s_off = io.type_off[tr.src_type];
        v_time = stamp_time(V.ty(tr.tgt_type).stamp[v]);
    }
    for (int p0 = 0; p0 < deg; p0 += G) {
        const int p = p0 + lane;
        int s = -1, ser = -1;
        if (p < deg) {
            s = tr.src[beg + p];
            if ((unsigned)s < (unsigned)S.n_nodes) ser = S.serial[s];
            if (ser < mk.src_below) ser = -1;
        }
        int total;
        const int prefix = group_scan_flag<G>(ser >= 0, &total, sh);
        if constexpr (FILL) {
            const int e = base + run + prefix;
            if (ser >= 0 && e >= 0 && e < io.n_edges) {
                io.src_out[e] = s_off + ser;
                io.dst_out[e] = tgt;
                io.time_out[e] = v_time - stamp_time(S.stamp[s]) + HGT_RTE_SELF;  // data.py:250
            }
        }
        run += total;
    }
    if constexpr (!FILL)
        if (lane == 0) io.rowoff[slot] = run;
}

template <bool FILL, bool BATCHED>
__device__ __forceinline__ void induce_rows(const View<BATCHED>& V, const Masks& mk, int n_slots, const InduceIO& io) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= n_slots) return;
    int m, i, v, deg;
    induce_decode(V, slot, &m, &i, &v, &deg);
    if (deg <= 0) {
        if (!FILL && lane == 0) io.rowoff[slot] = 0;
        return;
    }
    if (deg > HUB) {                                                              // the fill pass walks the queue the count pass wrote
        if (!FILL && lane == 0) {
            const int idx = atomicAdd(io.hub_n, 1);
            if (idx < n_slots) io.hub_rows[idx] = slot;
        }
        return;
    }
    induce_row<HGT_WAVE, FILL>(V, mk.m[m], m, i, v, deg, slot, lane, nullptr, io);
}

template <bool FILL, bool BATCHED>
__device__ __forceinline__ void induce_hub_rows(const View<BATCHED>& V, const Masks& mk, int n_slots, const InduceIO& io) {
    __shared__ int sh[BIG / HGT_WAVE];
    const int n = clamp0(*io.hub_n, n_slots);
    for (int h = blockIdx.x; h < n; h += gridDim.x) {
        const int slot = io.hub_rows[h];
        if ((unsigned)slot >= (unsigned)n_slots) continue;
        int m, i, v, deg;
        induce_decode(V, slot, &m, &i, &v, &deg);
        if (deg <= 0) continue;
        induce_row<BIG, FILL>(V, mk.m[m], m, i, v, deg, slot, threadIdx.x, sh, io);
    }
}

template <bool FILL>
__global__ void __launch_bounds__(256) k_induce(Tables tb, Masks mk, int n_slots, int32_t* __restrict__ rowoff, int32_t* __restrict__ hub,
                                                const int32_t* __restrict__ type_off, int32_t* __restrict__ src_out,
                                                int32_t* __restrict__ dst_out, int32_t* __restrict__ time_out, int n_edges) {
    induce_rows<FILL>(View<false>{tb, 0}, mk, n_slots, InduceIO{rowoff, hub, hub + 1, type_off, src_out, dst_out, time_out, n_edges});
}

template <bool FILL>
__global__ void __launch_bounds__(BIG) k_induce_hub(Tables tb, Masks mk, int n_slots, int32_t* __restrict__ rowoff, int32_t* __restrict__ hub,
                                                    const int32_t* __restrict__ type_off, int32_t* __restrict__ src_out,
                                                    int32_t* __restrict__ dst_out, int32_t* __restrict__ time_out, int n_edges) {
    induce_hub_rows<FILL>(View<false>{tb, 0}, mk, n_slots, InduceIO{rowoff, hub, hub + 1, type_off, src_out, dst_out, time_out, n_edges});
}

// the scratch and the outputs of a batched call; replica_io cuts replica b's part out of them (false: the fill pass has no valid range)
struct BatchIO {
    int32_t* rowoff;             // [B][stride]
    int32_t* hub;                // B counters, then [B][stride - 1] entries
    int64_t stride;
    const int32_t* type_off;     // [B][T + 1]
    const int32_t* offs;         // fill: node prefix sums [B + 1], edge prefix sums [B + 1]
    int32_t* src_out;
    int32_t* dst_out;
    int32_t* time_out;
    int n_nodes, n_edges;        // fill: totals over the replicas
};

template <bool FILL>
__device__ __forceinline__ bool replica_io(const BatchIO& io, int T, int b, int B, InduceIO* out) {
    *out = InduceIO{io.rowoff + b * io.stride, io.hub + b, io.hub + B + b * (io.stride - 1), nullptr, nullptr, nullptr, nullptr, 0};
    if constexpr (FILL) {
        Range r;
        if (!replica_range(io.offs, b, B, io.n_nodes, io.n_edges, &r)) return false;
        out->type_off = io.type_off + (int64_t)b * (T + 1);
        out->src_out = io.src_out + r.e0;
        out->dst_out = io.dst_out + r.e0;
        out->time_out = io.time_out + r.e0;
        out->n_edges = r.ne - r.nn;
    }
    return true;
}

template <bool FILL>
__global__ void __launch_bounds__(256) k_induce_batched(Tables tb, Masks mk, int n_slots, BatchIO bio) {
    InduceIO io;
    if (!replica_io<FILL>(bio, tb.T, blockIdx.y, gridDim.y, &io)) return;
    induce_rows<FILL>(View<true>{tb, (int)blockIdx.y}, mk, n_slots, io);
}

template <bool FILL>
__global__ void __launch_bounds__(BIG) k_induce_hub_batched(Tables tb, Masks mk, int n_slots, BatchIO bio) {
    InduceIO io;
    if (!replica_io<FILL>(bio, tb.T, blockIdx.y, gridDim.y, &io)) return;
    induce_hub_rows<FILL>(View<true>{tb, (int)blockIdx.y}, mk, n_slots, io);
}

// one workgroup: rowoff[] counts -> exclusive offsets (rowoff[n_slots] = number of non-self edges), type_off, rel_ptr, sizes
template <bool BATCHED>
__device__ __forceinline__ void induce_scan(const View<BATCHED>& V, int n_slots, int R, int32_t* __restrict__ rowoff, int32_t* __restrict__ type_off,
                                            int32_t* __restrict__ rel_ptr, int32_t* __restrict__ sizes) {
    __shared__ int32_t part[BIG];
    const Tables& tb = V.tb;
    const int k = threadIdx.x;
    const int chunk = (n_slots + BIG - 1) / BIG;
    const int beg = min(n_slots, k * chunk), end = min(n_slots, beg + chunk);
    int sum = 0;
    for (int i = beg; i < end; ++i) sum += rowoff[i];
    part[k] = sum;
    __syncthreads();
    for (int step = 1; step < BIG; step <<= 1) {
        const int add = k >= step ? part[k - step] : 0;
        __syncthreads();
        part[k] += add;
        __syncthreads();
    }
    int run = part[k] - sum;
    for (int i = beg; i < end; ++i) {
        const int c = rowoff[i];
        rowoff[i] = run;
        run += c;
    }
    if (k == BIG - 1) rowoff[n_slots] = part[BIG - 1];
    __syncthreads();
    const int T = tb.T, M = tb.M;
    const int e_ns = rowoff[n_slots];
    if (k == 0) {
        int n = 0, flag = 0;
        for (int t = 0; t < T; ++t) {
            const hgt_sampler_type S = V.ty(t);
            const int c = clamp0(S.counts[0], S.cap_sampled);
            type_off[t] = n;
            sizes[t] = c;
            n += c;
            flag |= S.counts[3];
        }
        type_off[T] = n;
        sizes[T + M] = flag;
        sizes[T + M + 1] = e_ns;
        rel_ptr[R] = e_ns + n;
    }
    if (k < M) sizes[T + k] = rowoff[tb.slot_off[k + 1]] - rowoff[tb.slot_off[k]];
    if (k < R) {                                                                  // triples are ordered by relation id; `self` = R - 1 is last
        int m = 0;
        while (m < M && tb.tr[m].rel_id < k) ++m;
        rel_ptr[k] = m < M ? rowoff[tb.slot_off[m]] : e_ns;
    }
}

__global__ void __launch_bounds__(BIG) k_induce_scan(Tables tb, int n_slots, int R, int32_t* __restrict__ rowoff, int32_t* __restrict__ type_off,
                                                     int32_t* __restrict__ rel_ptr, int32_t* __restrict__ sizes) {
    induce_scan(View<false>{tb, 0}, n_slots, R, rowoff, type_off, rel_ptr, sizes);
}

__global__ void __launch_bounds__(BIG) k_induce_scan_batched(Tables tb, int n_slots, int R, int32_t* __restrict__ rowoff, int64_t stride,
                                                             int32_t* __restrict__ type_off, int32_t* __restrict__ rel_ptr,
                                                             int32_t* __restrict__ sizes) {
    const int b = blockIdx.y;
    induce_scan(View<true>{tb, b}, n_slots, R, rowoff + b * stride, type_off + (int64_t)b * (tb.T + 1), rel_ptr + (int64_t)b * (R + 1),
                sizes + (int64_t)b * (tb.T + tb.M + 2));
}

// batched fill: sizes [B][T + M + 2] of the count pass -> offs = node prefix sums over b [B + 1], then edge prefix sums [B + 1]
__global__ void __launch_bounds__(64) k_batch_offsets(const int32_t* __restrict__ sizes, int B, int T, int M, int32_t* __restrict__ offs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t n = 0, e = 0;
    const int64_t top = 0x7fffffff;
    for (int b = 0; b < B; ++b) {
        const int32_t* s = sizes + (int64_t)b * (T + M + 2);
        offs[b] = (int32_t)n;
        offs[B + 1 + b] = (int32_t)e;
        int64_t nb = 0;
        for (int t = 0; t < T; ++t) nb += s[t] > 0 ? s[t] : 0;
        n += nb;
        e += nb + (s[T + M + 1] > 0 ? s[T + M + 1] : 0);
        if (n > top) n = top;
        if (e > top) e = top;
    }
    offs[B] = (int32_t)n;
    offs[2 * B + 1] = (int32_t)e;
}

// per sampled node: its `self` edge (data.py:183-186), its time and its original id, in global order
template <bool BATCHED>
__device__ __forceinline__ void induce_nodes(const View<BATCHED>& V, const int32_t* __restrict__ type_off, int e_ns, int n_edges, int n_nodes,
                                             int32_t* __restrict__ src_out, int32_t* __restrict__ dst_out, int32_t* __restrict__ time_out,
                                             int32_t* __restrict__ node_time, int32_t* __restrict__ node_id) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_nodes) return;
    int t = 0;
    while (t + 1 < V.tb.T && type_off[t + 1] <= g) ++t;
    const hgt_sampler_type S = V.ty(t);
    const int i = g - type_off[t];
    if (i < 0 || i >= S.cap_sampled) return;
    const int v = S.sampled[i];
    node_id[g] = v;
    node_time[g] = (unsigned)v < (unsigned)S.n_nodes ? stamp_time(S.stamp[v]) : 0;
    const int e = e_ns + g;
    if (e >= 0 && e < n_edges) {
        src_out[e] = g;
        dst_out[e] = g;
        time_out[e] = HGT_RTE_SELF;
    }
}

__global__ void __launch_bounds__(256) k_induce_nodes(Tables tb, const int32_t* __restrict__ type_off, int e_ns, int n_edges, int n_nodes,
                                                      int32_t* __restrict__ src_out, int32_t* __restrict__ dst_out, int32_t* __restrict__ time_out,
                                                      int32_t* __restrict__ node_time, int32_t* __restrict__ node_id) {
    induce_nodes(View<false>{tb, 0}, type_off, e_ns, n_edges, n_nodes, src_out, dst_out, time_out, node_time, node_id);
}

__global__ void __launch_bounds__(256) k_induce_nodes_batched(Tables tb, const int32_t* __restrict__ type_off, const int32_t* __restrict__ offs,
                                                              int n_edges, int n_nodes, int32_t* __restrict__ src_out,
                                                              int32_t* __restrict__ dst_out, int32_t* __restrict__ time_out,
                                                              int32_t* __restrict__ node_time, int32_t* __restrict__ node_id) {
    const int b = blockIdx.y;
    Range r;
    if (!replica_range(offs, b, gridDim.y, n_nodes, n_edges, &r)) return;
    induce_nodes(View<true>{tb, b}, type_off + (int64_t)b * (tb.T + 1), r.ne - r.nn, r.ne, r.nn, src_out + r.e0, dst_out + r.e0, time_out + r.e0,
                 node_time + r.n0, node_id + r.n0);
}

// ------------------------------------------------------------------------------------------------ features of a batched call
struct Features {
    const float* f[HGT_SAMPLER_MAX_TYPES];
    int32_t n[HGT_SAMPLER_MAX_TYPES];
};

// one wavefront per output row g: replica from the node prefix sums, type from the replica's type_off, then a copy of the row
__global__ void __launch_bounds__(256) k_gather_features(Features F, int T, int B, int width, const int32_t* __restrict__ type_off,
                                                         const int32_t* __restrict__ offs, const int32_t* __restrict__ node_id, int n_rows,
                                                         float* __restrict__ out, int vec) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_rows) return;
    int lo = 0, hi = B - 1;                                                       // the last replica whose first row is <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int local = g - offs[lo];
    if (local < 0 || g >= offs[lo + 1]) return;
    const int32_t* to = type_off + (int64_t)lo * (T + 1);
    int t = 0;
    while (t + 1 < T && to[t + 1] <= local) ++t;
    const int v = node_id[g];
    const float* __restrict__ row = F.f[t];
    if (!row || (unsigned)v >= (unsigned)F.n[t]) return;
    row += (int64_t)v * width;
    float* __restrict__ dst = out + (int64_t)g * width;
    if (vec) {                                                                    // rows of both sides start on 16 bytes
        for (int c = lane; c < (width >> 2); c += HGT_WAVE) ((float4*)dst)[c] = ((const float4*)row)[c];
    } else {
        for (int c = lane; c < width; c += HGT_WAVE) dst[c] = row[c];
    }
}

// ------------------------------------------------------------------------------------------------ reset
template <bool BATCHED>
__device__ __forceinline__ void reset_nodes(const View<BATCHED>& V) {
    const int stride = gridDim.x * blockDim.x, i0 = blockIdx.x * blockDim.x + threadIdx.x;
    for (int t = 0; t < V.tb.T; ++t) {
        const hgt_sampler_type S = V.ty(t);
        const int ns = clamp0(S.counts[0], S.cap_sampled), nc = clamp0(S.counts[2], S.cap_cand);
        for (int i = i0; i < ns + nc; i += stride) {
            const int v = i < ns ? S.sampled[i] : S.cand[i - ns];
            if ((unsigned)v >= (unsigned)S.n_nodes) continue;
            S.score[v] = 0ull;
            S.stamp[v] = 0ull;
            S.serial[v] = -1;
        }
    }
}

template <bool BATCHED>
__device__ __forceinline__ void reset_counts(const View<BATCHED>& V) {
    const int i = threadIdx.x;
    if (i < V.tb.T * 4) V.ty(i >> 2).counts[i & 3] = 0;
}

__global__ void __launch_bounds__(256) k_reset_nodes(Tables tb) { reset_nodes(View<false>{tb, 0}); }
__global__ void __launch_bounds__(64) k_reset_counts(Tables tb) { reset_counts(View<false>{tb, 0}); }
__global__ void __launch_bounds__(256) k_reset_nodes_batched(Tables tb) { reset_nodes(View<true>{tb, (int)blockIdx.y}); }
__global__ void __launch_bounds__(64) k_reset_counts_batched(Tables tb) { reset_counts(View<true>{tb, (int)blockIdx.y}); }

// ------------------------------------------------------------------------------------------------ host side
// validates the tables and copies them into the kernel-argument form; slot_off is filled for the induce calls
int make_tables(const hgt_sampler_type* types, int32_t T, const hgt_sampler_triple* triples, int32_t M, Tables* out, int64_t* n_slots) {
    if (!types || T < 1 || M < 0 || (M > 0 && !triples)) return HGT_ERR_INVALID_ARG;
    if (T > HGT_SAMPLER_MAX_TYPES || M > HGT_SAMPLER_MAX_TRIPLES) return HGT_ERR_UNSUPPORTED;
    Tables& tb = *out;
    tb.T = T;
    tb.M = M;
    for (int t = 0; t < HGT_SAMPLER_MAX_TYPES; ++t) tb.ty[t] = types[t < T ? t : T - 1];
    for (int t = 0; t < T; ++t) {
        const hgt_sampler_type& S = types[t];
        if (S.n_nodes < 0 || S.cap_sampled < 0 || S.cap_cand < 0 || !S.counts) return HGT_ERR_INVALID_ARG;
        if (S.n_nodes > 0 && (!S.score || !S.stamp || !S.serial)) return HGT_ERR_INVALID_ARG;
        if ((S.cap_sampled > 0 && !S.sampled) || (S.cap_cand > 0 && !S.cand)) return HGT_ERR_INVALID_ARG;
        if (S.cap_sampled > S.n_nodes || S.cap_cand > S.n_nodes) return HGT_ERR_INVALID_ARG;
    }
    int64_t slots = 0;
    for (int m = 0; m < HGT_SAMPLER_MAX_TRIPLES; ++m) {
        if (m < M) {
            const hgt_sampler_triple& tr = triples[m];
            if (tr.tgt_type < 0 || tr.tgt_type >= T || tr.src_type < 0 || tr.src_type >= T || tr.rel_id < 0) return HGT_ERR_INVALID_ARG;
            if (!tr.indptr) return HGT_ERR_INVALID_ARG;      // [n_tgt + 1] entries even for an empty type
            tb.tr[m] = tr;
            tb.slot_off[m] = (int32_t)slots;
            slots += types[tr.tgt_type].cap_sampled;
            if (slots > 0x3fffffff) return HGT_ERR_TOO_LARGE;
        } else {
            tb.tr[m] = hgt_sampler_triple{nullptr, nullptr, nullptr, 0, 0, 0, 0};
            tb.slot_off[m] = (int32_t)slots;
        }
    }
    tb.slot_off[HGT_SAMPLER_MAX_TRIPLES] = (int32_t)slots;
    if (M < HGT_SAMPLER_MAX_TRIPLES) tb.slot_off[M] = (int32_t)slots;
    if (n_slots) *n_slots = slots;
    return HGT_OK;
}

inline unsigned blocks_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

constexpr int HUB_BLOCKS = 256;      // workgroups of the hub launches: each loops over the queue

}  // namespace

// One host body per step, for the single entry points (BATCHED = false: n_batch is 1, the Philox key is `seed`) and the batched ones
// (include/hgt_hip.h, "Batched device sampler": n_batch replicas in gridDim.y of the launches of one batch, the keys from seeds_host).
// Both run the same checks in the same order; `if constexpr` stands around what differs: batch_check and make_keys, which wrapper is
// launched with which trailing arguments, and in the fill pass the offsets launch and BatchIO.
static int batch_check(int32_t n_batch) {
    if (n_batch < 1) return HGT_ERR_INVALID_ARG;
    if (n_batch > HGT_SAMPLER_MAX_BATCH) return HGT_ERR_UNSUPPORTED;
    return HGT_OK;
}

static int make_keys(const uint64_t* seeds_host, int32_t n_batch, Keys* out) {
    if (!seeds_host) return HGT_ERR_INVALID_ARG;
    for (int b = 0; b < HGT_SAMPLER_MAX_BATCH; ++b) {
        const uint64_t seed = b < n_batch ? seeds_host[b] : 0;
        out->k[b][0] = (uint32_t)seed;
        out->k[b][1] = (uint32_t)(seed >> 32);
    }
    return HGT_OK;
}

template <bool BATCHED>
static int seed_step(const hgt_sampler_type* types_host, int32_t n_types, int32_t n_batch, int32_t type, const int32_t* ids,
                      const int32_t* times, int32_t n, int32_t step, void* stream) {
    Tables tb;
    if (int rc = make_tables(types_host, n_types, nullptr, 0, &tb, nullptr)) return rc;
    if constexpr (BATCHED)
        if (int rc = batch_check(n_batch)) return rc;
    if (type < 0 || type >= n_types || n < 0 || step < 0) return HGT_ERR_INVALID_ARG;
    if (n > types_host[type].cap_sampled) return HGT_ERR_WORKSPACE;
    if (n > 0 && (!ids || !times)) return HGT_ERR_INVALID_ARG;
    (BATCHED ? k_seed_batched : k_seed)<<<dim3(blocks_for(n > 0 ? n : 1, 256), n_batch), 256, 0, (hipStream_t)stream>>>(tb, type, ids, times, n, step);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

template <bool BATCHED>
static int budget_step(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host, int32_t n_triples,
                      int32_t n_batch, int32_t type, int32_t step, int32_t sampled_number, int32_t max_new, int32_t has_max_time,
                      int32_t max_time, uint64_t seed, const uint64_t* seeds_host, int32_t* hub, int64_t hub_entries, void* stream) {
    Tables tb;
    Keys keys;
    if (int rc = make_tables(types_host, n_types, triples_host, n_triples, &tb, nullptr)) return rc;
    if constexpr (BATCHED) {
        if (int rc = batch_check(n_batch)) return rc;
        if (int rc = make_keys(seeds_host, n_batch, &keys)) return rc;
    }
    if (type < 0 || type >= n_types || step < 0 || sampled_number < 1 || max_new < 0) return HGT_ERR_INVALID_ARG;
    if (sampled_number > HGT_SAMPLER_MAX_NUMBER) return HGT_ERR_UNSUPPORTED;
    BudgetParams P;
    P.t = type; P.step = step; P.sn = sampled_number; P.has_max = has_max_time != 0; P.max_time = max_time; P.max_new = max_new;
    P.k0 = BATCHED ? 0 : (uint32_t)seed;                      // batched: the replicas' keys ride in `keys`
    P.k1 = BATCHED ? 0 : (uint32_t)(seed >> 32);
    P.ntr = 0;
    for (int m = 0; m < HGT_SAMPLER_MAX_TRIPLES; ++m) P.sel[m] = 0;
    for (int m = 0; m < n_triples; ++m) {
        if (triples_host[m].tgt_type != type) continue;
        const hgt_sampler_triple& tr = triples_host[m];
        if (types_host[tr.src_type].n_nodes > 0 && types_host[type].n_nodes > 0 && (!tr.src || !tr.time)) return HGT_ERR_INVALID_ARG;
        P.sel[P.ntr++] = (uint8_t)m;
    }
    const int64_t rows = (int64_t)max_new * P.ntr;
    if (rows == 0) return HGT_OK;
    if (rows > 0x3fffffff) return HGT_ERR_TOO_LARGE;
    if (!hub) return HGT_ERR_INVALID_ARG;
    if (hub_entries < rows + 1) return HGT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hub, 0, 4 * (size_t)n_batch, st) != hipSuccess) return HGT_ERR_LAUNCH;
    const dim3 grid(blocks_for(rows, 4), n_batch), hub_grid((unsigned)(rows < HUB_BLOCKS ? rows : HUB_BLOCKS), n_batch);
    if constexpr (BATCHED) {
        k_budget_batched<<<grid, 256, 0, st>>>(tb, P, keys, hub, hub_entries - 1, (int)rows);
        HGT_CHECK_LAUNCH();
        k_budget_hub_batched<<<hub_grid, BIG, 0, st>>>(tb, P, keys, hub, hub_entries - 1, (int)rows);
    } else {
        k_budget<<<grid, 256, 0, st>>>(tb, P, hub, (int)rows);
        HGT_CHECK_LAUNCH();
        k_budget_hub<<<hub_grid, BIG, 0, st>>>(tb, P, hub, (int)rows);
    }
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

template <bool BATCHED>
static int select_step(const hgt_sampler_type* types_host, int32_t n_types, int32_t n_batch, int32_t type, int32_t step, int32_t sampled_number,
                  uint64_t seed, const uint64_t* seeds_host, uint64_t* keys, int32_t* tmp, int64_t tmp_entries, void* stream) {
    Tables tb;
    Keys seeds;
    if (int rc = make_tables(types_host, n_types, nullptr, 0, &tb, nullptr)) return rc;
    if constexpr (BATCHED) {
        if (int rc = batch_check(n_batch)) return rc;
        if (int rc = make_keys(seeds_host, n_batch, &seeds)) return rc;
    }
    if (type < 0 || type >= n_types || step < 0 || sampled_number < 1) return HGT_ERR_INVALID_ARG;
    if (sampled_number > HGT_SAMPLER_MAX_NUMBER) return HGT_ERR_UNSUPPORTED;
    const int cap = types_host[type].cap_cand;
    if (cap == 0) return HGT_OK;
    if (!keys || !tmp) return HGT_ERR_INVALID_ARG;
    if (tmp_entries < cap) return HGT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks_for(cap, 256), n_batch), pick_grid(1, n_batch);
    if constexpr (BATCHED) {
        k_select_keys_batched<<<grid, 256, 0, st>>>(tb, type, step, seeds, keys, tmp_entries);
        HGT_CHECK_LAUNCH();
        k_select_pick_batched<<<pick_grid, BIG, 0, st>>>(tb, type, sampled_number, keys, tmp, tmp_entries);
    } else {
        k_select_keys<<<grid, 256, 0, st>>>(tb, type, step, (uint32_t)seed, (uint32_t)(seed >> 32), keys);
        HGT_CHECK_LAUNCH();
        k_select_pick<<<pick_grid, BIG, 0, st>>>(tb, type, sampled_number, keys, tmp);
    }
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

static int induce_check(const hgt_sampler_type* types_host, int32_t T, const hgt_sampler_triple* triples_host, int32_t M, int32_t R, Tables* tb,
                        int64_t* slots) {
    if (int rc = make_tables(types_host, T, triples_host, M, tb, slots)) return rc;
    if (R < 1 || R > HGT_SAMPLER_MAX_TRIPLES + 1) return HGT_ERR_INVALID_ARG;
    for (int m = 0; m < M; ++m) {
        const hgt_sampler_triple& tr = triples_host[m];
        if (tr.rel_id >= R - 1 || (m > 0 && tr.rel_id < triples_host[m - 1].rel_id)) return HGT_ERR_INVALID_ARG;
        if (m > 0 && tr.rel_id == triples_host[m - 1].rel_id && tr.tgt_type < triples_host[m - 1].tgt_type) return HGT_ERR_INVALID_ARG;
        if (types_host[tr.src_type].n_nodes > 0 && types_host[tr.tgt_type].n_nodes > 0 && !tr.src) return HGT_ERR_INVALID_ARG;
    }
    return HGT_OK;
}

// the thresholds of a masked call in kernel-argument form; masks_host == NULL with masked = false: the all-zero masks of the unmasked
// entry points, which run the same kernels
static int make_masks(const hgt_sampler_mask* masks_host, int32_t M, bool masked, Masks* out) {
    for (int m = 0; m < HGT_SAMPLER_MAX_TRIPLES; ++m) out->m[m] = hgt_sampler_mask{0, 0};
    if (!masked) return HGT_OK;
    if (!masks_host) return HGT_ERR_INVALID_ARG;
    for (int m = 0; m < M; ++m) {
        if (masks_host[m].tgt_below < 0 || masks_host[m].src_below < 0) return HGT_ERR_INVALID_ARG;
        out->m[m] = masks_host[m];
    }
    return HGT_OK;
}

// batched: the hub queues of the induce passes are n_batch counters, then n_entries - 1 >= slots entries per replica
template <bool BATCHED>
static int count_step(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host, int32_t n_triples,
                        int32_t n_batch, int32_t n_relations, int32_t* rowoff, int32_t* hub, int64_t n_entries, int32_t* type_off_out,
                        int32_t* rel_ptr_out, int32_t* sizes_out, const hgt_sampler_mask* masks_host, bool masked, void* stream) {
    Tables tb;
    Masks mk;
    int64_t slots = 0;
    if (int rc = induce_check(types_host, n_types, triples_host, n_triples, n_relations, &tb, &slots)) return rc;
    if constexpr (BATCHED)
        if (int rc = batch_check(n_batch)) return rc;
    if (int rc = make_masks(masks_host, n_triples, masked, &mk)) return rc;
    if (!rowoff || !hub || !type_off_out || !rel_ptr_out || !sizes_out) return HGT_ERR_INVALID_ARG;
    if (n_entries < slots + 1) return HGT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hub, 0, 4 * (size_t)n_batch, st) != hipSuccess) return HGT_ERR_LAUNCH;
    const dim3 grid(blocks_for(slots, 4), n_batch), hub_grid((unsigned)(slots < HUB_BLOCKS ? slots : HUB_BLOCKS), n_batch), scan_grid(1, n_batch);
    if constexpr (BATCHED) {
        const BatchIO io{rowoff, hub, n_entries, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
        if (slots > 0) {
            k_induce_batched<false><<<grid, 256, 0, st>>>(tb, mk, (int)slots, io);
            HGT_CHECK_LAUNCH();
            k_induce_hub_batched<false><<<hub_grid, BIG, 0, st>>>(tb, mk, (int)slots, io);
            HGT_CHECK_LAUNCH();
        }
        k_induce_scan_batched<<<scan_grid, BIG, 0, st>>>(tb, (int)slots, n_relations, rowoff, n_entries, type_off_out, rel_ptr_out, sizes_out);
    } else {
        if (slots > 0) {
            k_induce<false><<<grid, 256, 0, st>>>(tb, mk, (int)slots, rowoff, hub, nullptr, nullptr, nullptr, nullptr, 0);
            HGT_CHECK_LAUNCH();
            k_induce_hub<false><<<hub_grid, BIG, 0, st>>>(tb, mk, (int)slots, rowoff, hub, nullptr, nullptr, nullptr, nullptr, 0);
            HGT_CHECK_LAUNCH();
        }
        k_induce_scan<<<scan_grid, BIG, 0, st>>>(tb, (int)slots, n_relations, rowoff, type_off_out, rel_ptr_out, sizes_out);
    }
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

// sizes and offs_out: the batched call's (the count pass's sizes, the prefix sums the fill pass writes first); NULL in the single one
template <bool BATCHED>
static int fill_step(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host, int32_t n_triples,
                       int32_t n_batch, int32_t n_relations, const int32_t* rowoff, const int32_t* hub, int64_t n_entries,
                       const int32_t* type_off, const int32_t* sizes, int32_t* offs_out, int64_t n_nodes, int64_t n_edges, int32_t* src_out,
                       int32_t* dst_out, int32_t* time_out, int32_t* node_time_out, int32_t* node_id_out, const hgt_sampler_mask* masks_host,
                       bool masked, void* stream) {
    Tables tb;
    Masks mk;
    int64_t slots = 0;
    if (int rc = induce_check(types_host, n_types, triples_host, n_triples, n_relations, &tb, &slots)) return rc;
    if constexpr (BATCHED)
        if (int rc = batch_check(n_batch)) return rc;
    if (int rc = make_masks(masks_host, n_triples, masked, &mk)) return rc;
    if (!rowoff || !hub || !type_off || (BATCHED && (!sizes || !offs_out)) || n_nodes < 0 || n_edges < n_nodes) return HGT_ERR_INVALID_ARG;
    if (n_edges > 0x7fffffff) return HGT_ERR_TOO_LARGE;
    if (n_entries < slots + 1) return HGT_ERR_WORKSPACE;
    if (n_edges > 0 && (!src_out || !dst_out || !time_out)) return HGT_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!node_time_out || !node_id_out)) return HGT_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    int32_t* ro = const_cast<int32_t*>(rowoff);              // the FILL instantiations only read the scratch
    int32_t* hb = const_cast<int32_t*>(hub);
    const int e_ns = (int)(n_edges - n_nodes);
    const bool edges = slots > 0 && e_ns > 0;
    const dim3 grid(blocks_for(slots, 4), n_batch), hub_grid((unsigned)(slots < HUB_BLOCKS ? slots : HUB_BLOCKS), n_batch);
    if constexpr (BATCHED) {
        k_batch_offsets<<<1, 64, 0, st>>>(sizes, n_batch, n_types, n_triples, offs_out);
        HGT_CHECK_LAUNCH();
        const BatchIO io{ro, hb, n_entries, type_off, offs_out, src_out, dst_out, time_out, (int)n_nodes, (int)n_edges};
        if (edges) {
            k_induce_batched<true><<<grid, 256, 0, st>>>(tb, mk, (int)slots, io);
            HGT_CHECK_LAUNCH();
            k_induce_hub_batched<true><<<hub_grid, BIG, 0, st>>>(tb, mk, (int)slots, io);
            HGT_CHECK_LAUNCH();
        }
        if (n_nodes > 0) {
            int64_t cap = 0;                                  // no replica has more nodes than the lists hold
            for (int t = 0; t < n_types; ++t) cap += types_host[t].cap_sampled;
            if (cap > n_nodes) cap = n_nodes;
            k_induce_nodes_batched<<<dim3(blocks_for(cap > 0 ? cap : 1, 256), n_batch), 256, 0, st>>>(
                tb, type_off, offs_out, (int)n_edges, (int)n_nodes, src_out, dst_out, time_out, node_time_out, node_id_out);
            HGT_CHECK_LAUNCH();
        }
    } else {
        if (edges) {
            k_induce<true><<<grid, 256, 0, st>>>(tb, mk, (int)slots, ro, hb, type_off, src_out, dst_out, time_out, e_ns);
            HGT_CHECK_LAUNCH();
            k_induce_hub<true><<<hub_grid, BIG, 0, st>>>(tb, mk, (int)slots, ro, hb, type_off, src_out, dst_out, time_out, e_ns);
            HGT_CHECK_LAUNCH();
        }
        if (n_nodes > 0) {
            k_induce_nodes<<<blocks_for(n_nodes, 256), 256, 0, st>>>(tb, type_off, e_ns, (int)n_edges, (int)n_nodes, src_out, dst_out, time_out,
                                                                     node_time_out, node_id_out);
            HGT_CHECK_LAUNCH();
        }
    }
    return HGT_OK;
}

template <bool BATCHED>
static int reset_step(const hgt_sampler_type* types_host, int32_t n_types, int32_t n_batch, void* stream) {
    Tables tb;
    if (int rc = make_tables(types_host, n_types, nullptr, 0, &tb, nullptr)) return rc;
    if constexpr (BATCHED)
        if (int rc = batch_check(n_batch)) return rc;
    hipStream_t st = (hipStream_t)stream;
    (BATCHED ? k_reset_nodes_batched : k_reset_nodes)<<<dim3(256, n_batch), 256, 0, st>>>(tb);
    HGT_CHECK_LAUNCH();
    (BATCHED ? k_reset_counts_batched : k_reset_counts)<<<dim3(1, n_batch), 64, 0, st>>>(tb);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

// ------------------------------------------------------------------------------------------------ the exported step functions: forwarders
// The single entry points stand before the batched ones: that is the order in which the k_induce* templates are first needed, and
// so the order of the kernels in the code object.
extern "C" int hgt_sampler_seed(const hgt_sampler_type* types_host, int32_t n_types, int32_t type, const int32_t* ids, const int32_t* times,
                                int32_t n, int32_t step, void* stream) {
    return seed_step<false>(types_host, n_types, 1, type, ids, times, n, step, stream);
}

extern "C" int hgt_sampler_add_budget(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                      int32_t n_triples, int32_t type, int32_t step, int32_t sampled_number, int32_t max_new,
                                      int32_t has_max_time, int32_t max_time, uint64_t seed, int32_t* hub, int64_t hub_entries, void* stream) {
    return budget_step<false>(types_host, n_types, triples_host, n_triples, 1, type, step, sampled_number, max_new, has_max_time, max_time, seed,
                             nullptr, hub, hub_entries, stream);
}

extern "C" int hgt_sampler_select(const hgt_sampler_type* types_host, int32_t n_types, int32_t type, int32_t step, int32_t sampled_number,
                                  uint64_t seed, uint64_t* keys, int32_t* tmp, int64_t tmp_entries, void* stream) {
    return select_step<false>(types_host, n_types, 1, type, step, sampled_number, seed, nullptr, keys, tmp, tmp_entries, stream);
}

extern "C" int hgt_sampler_induce_slots(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                        int32_t n_triples, int64_t* n_slots_host) {
    Tables tb;
    if (!n_slots_host) return HGT_ERR_INVALID_ARG;
    return make_tables(types_host, n_types, triples_host, n_triples, &tb, n_slots_host);
}

extern "C" int hgt_sampler_induce_count(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                        int32_t n_triples, int32_t n_relations, int32_t* rowoff, int32_t* hub, int64_t n_entries,
                                        int32_t* type_off_out, int32_t* rel_ptr_out, int32_t* sizes_out, void* stream) {
    return count_step<false>(types_host, n_types, triples_host, n_triples, 1, n_relations, rowoff, hub, n_entries, type_off_out, rel_ptr_out,
                               sizes_out, nullptr, false, stream);
}

extern "C" int hgt_sampler_induce_count_masked(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                               int32_t n_triples, int32_t n_relations, int32_t* rowoff, int32_t* hub, int64_t n_entries,
                                               int32_t* type_off_out, int32_t* rel_ptr_out, int32_t* sizes_out,
                                               const hgt_sampler_mask* masks_host, void* stream) {
    return count_step<false>(types_host, n_types, triples_host, n_triples, 1, n_relations, rowoff, hub, n_entries, type_off_out, rel_ptr_out,
                               sizes_out, masks_host, true, stream);
}

extern "C" int hgt_sampler_induce_fill(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                       int32_t n_triples, int32_t n_relations, const int32_t* rowoff, const int32_t* hub, int64_t n_entries,
                                       const int32_t* type_off, int64_t n_nodes, int64_t n_edges, int32_t* src_out, int32_t* dst_out,
                                       int32_t* time_out, int32_t* node_time_out, int32_t* node_id_out, void* stream) {
    return fill_step<false>(types_host, n_types, triples_host, n_triples, 1, n_relations, rowoff, hub, n_entries, type_off, nullptr, nullptr,
                              n_nodes, n_edges, src_out, dst_out, time_out, node_time_out, node_id_out, nullptr, false, stream);
}

extern "C" int hgt_sampler_induce_fill_masked(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                              int32_t n_triples, int32_t n_relations, const int32_t* rowoff, const int32_t* hub,
                                              int64_t n_entries, const int32_t* type_off, int64_t n_nodes, int64_t n_edges, int32_t* src_out,
                                              int32_t* dst_out, int32_t* time_out, int32_t* node_time_out, int32_t* node_id_out,
                                              const hgt_sampler_mask* masks_host, void* stream) {
    return fill_step<false>(types_host, n_types, triples_host, n_triples, 1, n_relations, rowoff, hub, n_entries, type_off, nullptr, nullptr,
                              n_nodes, n_edges, src_out, dst_out, time_out, node_time_out, node_id_out, masks_host, true, stream);
}

extern "C" int hgt_sampler_reset(const hgt_sampler_type* types_host, int32_t n_types, void* stream) {
    return reset_step<false>(types_host, n_types, 1, stream);
}

extern "C" int hgt_sampler_seed_batched(const hgt_sampler_type* types_host, int32_t n_types, int32_t n_batch, int32_t type, const int32_t* ids,
                                        const int32_t* times, int32_t n, int32_t step, void* stream) {
    return seed_step<true>(types_host, n_types, n_batch, type, ids, times, n, step, stream);
}

extern "C" int hgt_sampler_add_budget_batched(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                              int32_t n_triples, int32_t n_batch, int32_t type, int32_t step, int32_t sampled_number,
                                              int32_t max_new, int32_t has_max_time, int32_t max_time, const uint64_t* seeds_host, int32_t* hub,
                                              int64_t hub_entries, void* stream) {
    return budget_step<true>(types_host, n_types, triples_host, n_triples, n_batch, type, step, sampled_number, max_new, has_max_time, max_time, 0,
                            seeds_host, hub, hub_entries, stream);
}

extern "C" int hgt_sampler_select_batched(const hgt_sampler_type* types_host, int32_t n_types, int32_t n_batch, int32_t type, int32_t step,
                                          int32_t sampled_number, const uint64_t* seeds_host, uint64_t* keys, int32_t* tmp, int64_t tmp_entries,
                                          void* stream) {
    return select_step<true>(types_host, n_types, n_batch, type, step, sampled_number, 0, seeds_host, keys, tmp, tmp_entries, stream);
}

extern "C" int hgt_sampler_induce_count_batched(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                                int32_t n_triples, int32_t n_batch, int32_t n_relations, int32_t* rowoff, int32_t* hub,
                                                int64_t n_entries, int32_t* type_off_out, int32_t* rel_ptr_out, int32_t* sizes_out,
                                                void* stream) {
    return count_step<true>(types_host, n_types, triples_host, n_triples, n_batch, n_relations, rowoff, hub, n_entries, type_off_out,
                              rel_ptr_out, sizes_out, nullptr, false, stream);
}

extern "C" int hgt_sampler_induce_count_masked_batched(const hgt_sampler_type* types_host, int32_t n_types,
                                                       const hgt_sampler_triple* triples_host, int32_t n_triples, int32_t n_batch,
                                                       int32_t n_relations, int32_t* rowoff, int32_t* hub, int64_t n_entries,
                                                       int32_t* type_off_out, int32_t* rel_ptr_out, int32_t* sizes_out,
                                                       const hgt_sampler_mask* masks_host, void* stream) {
    return count_step<true>(types_host, n_types, triples_host, n_triples, n_batch, n_relations, rowoff, hub, n_entries, type_off_out,
                              rel_ptr_out, sizes_out, masks_host, true, stream);
}

extern "C" int hgt_sampler_induce_fill_batched(const hgt_sampler_type* types_host, int32_t n_types, const hgt_sampler_triple* triples_host,
                                               int32_t n_triples, int32_t n_batch, int32_t n_relations, const int32_t* rowoff,
                                               const int32_t* hub, int64_t n_entries, const int32_t* type_off, const int32_t* sizes,
                                               int32_t* offs_out, int64_t n_nodes, int64_t n_edges, int32_t* src_out, int32_t* dst_out,
                                               int32_t* time_out, int32_t* node_time_out, int32_t* node_id_out, void* stream) {
    return fill_step<true>(types_host, n_types, triples_host, n_triples, n_batch, n_relations, rowoff, hub, n_entries, type_off, sizes,
                             offs_out, n_nodes, n_edges, src_out, dst_out, time_out, node_time_out, node_id_out, nullptr, false, stream);
}

extern "C" int hgt_sampler_induce_fill_masked_batched(const hgt_sampler_type* types_host, int32_t n_types,
                                                      const hgt_sampler_triple* triples_host, int32_t n_triples, int32_t n_batch,
                                                      int32_t n_relations, const int32_t* rowoff, const int32_t* hub, int64_t n_entries,
                                                      const int32_t* type_off, const int32_t* sizes, int32_t* offs_out, int64_t n_nodes,
                                                      int64_t n_edges, int32_t* src_out, int32_t* dst_out, int32_t* time_out,
                                                      int32_t* node_time_out, int32_t* node_id_out, const hgt_sampler_mask* masks_host,
                                                      void* stream) {
    return fill_step<true>(types_host, n_types, triples_host, n_triples, n_batch, n_relations, rowoff, hub, n_entries, type_off, sizes,
                             offs_out, n_nodes, n_edges, src_out, dst_out, time_out, node_time_out, node_id_out, masks_host, true, stream);
}

extern "C" int hgt_sampler_reset_batched(const hgt_sampler_type* types_host, int32_t n_types, int32_t n_batch, void* stream) {
    return reset_step<true>(types_host, n_types, n_batch, stream);
}

extern "C" int hgt_sampler_gather_features(const float* const* features_host, const int32_t* type_nodes_host, int32_t n_types, int32_t n_batch,
                                           int32_t width, const int32_t* type_off, const int32_t* offs, const int32_t* node_id, int64_t n_nodes,
                                           float* out, void* stream) {
    if (!features_host || !type_nodes_host || n_types < 1 || width < 0 || n_nodes < 0) return HGT_ERR_INVALID_ARG;
    if (n_types > HGT_SAMPLER_MAX_TYPES) return HGT_ERR_UNSUPPORTED;
    if (int rc = batch_check(n_batch)) return rc;
    if (n_nodes > 0x7fffffff / 4) return HGT_ERR_TOO_LARGE;
    Features F;
    for (int t = 0; t < HGT_SAMPLER_MAX_TYPES; ++t) {
        F.f[t] = t < n_types ? features_host[t] : nullptr;
        F.n[t] = t < n_types ? type_nodes_host[t] : 0;
        if (F.n[t] < 0) return HGT_ERR_INVALID_ARG;
    }
    if (n_nodes == 0 || width == 0) return HGT_OK;
    if (!type_off || !offs || !node_id || !out) return HGT_ERR_INVALID_ARG;
    uintptr_t bits = (uintptr_t)out | (uintptr_t)(width & 3);
    for (int t = 0; t < n_types; ++t) bits |= (uintptr_t)F.f[t];
    const int vec = (bits & 15) == 0;                         // every row of every matrix and of `out` starts on 16 bytes
    k_gather_features<<<blocks_for(n_nodes, 4), 256, 0, (hipStream_t)stream>>>(F, n_types, n_batch, width, type_off, offs, node_id, (int)n_nodes, out, vec);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}
