// Scoring a task batch on the device (gfx950): what the reference's training scripts do with a model's output after the step.
//
//   hgt_rank_metrics           NDCG@k and the reciprocal rank of every row of scores (OAG/train_paper_field.py:272-275, 303-308 and the
//                              venue / author scripts: one argsort row at a time, copied to the host, then pyHGT/utils.py:5-20)
//   hgt_segment_first_nll      mask_softmax of OAG/train_author_disambiguation.py:90-96: per segment (logsumexp - first) / ln(length)
//   hgt_segment_first_nll_bwd  its gradient
//
// Ranks (0-based, a tie goes to the lower position; s = scores, l = relevances of one row of C positions, positive = l > 0):
//   score rank of p   #{ j : s_j > s_p or (s_j == s_p and j < p) }
//   ideal rank of p   #{ j : l_j > l_p or (l_j == l_p and j < p) }
//   w(0) = 1, w(i) = 1 / log2(i + 1);  K = k > 0 ? k : C
//   DCG = sum over positives with rank < K of l_p * w(rank_p), IDCG the same over the ideal ranks, ndcg = DCG / IDCG (0 when IDCG == 0),
//   rr = 1 / (1 + min over positives of rank_p) (0 without a positive).  A NaN score in the row: both NaN.
//
// No sort: a rank is a count.  The positives of a row sit in an LDS list of HGT_RANK_LIST_CAP entries (position order); the row is
// streamed past the list and both counts of every entry come out as integers -- in registers, joined by integer adds in LDS.  A row with
// more positives takes further passes, each over the next HGT_RANK_LIST_CAP positives: the list is filled by one walk over the row that
// resumes where the last pass stopped, the counts by one stream of the row per pass, so there is no P^2 phase and no cap on P.  The l * w
// terms are formed in fp64 from the integer ranks and summed in an order the list fixes (entry i by thread i % 256, a shuffle tree, the
// four wavefront sums in order, pass after pass): no float atomic, and a row's bits depend on nothing outside the row.
//
// Rows of at most 64 positions (the author segments) take a wavefront each: lane p holds position p and counts its own two ranks over
// C shuffles.  Longer rows take a workgroup each; with a ragged call both kernels are launched and each row is written by exactly one.
//
// The loss kernels keep torch.log_softmax's arithmetic (fp32, x - max - log(sum exp(x - max))) and save the two parts (max, log sum) per
// segment so that the backward forms the same difference.  Compiled without fast-math like the rest of the library.
#include <limits.h>
#include <math.h>

#include "hgt_common.h"

namespace {

constexpr int TM_BLOCK = 256;
constexpr int TM_WAVES = TM_BLOCK / 64;
constexpr int TM_TILE = 4 * TM_BLOCK;                   // positions a step of the stream covers: four consecutive ones per thread
constexpr int TM_CAP = HGT_RANK_LIST_CAP;               // 5 arrays of 4 bytes: 20 KB of LDS
constexpr int TM_SMALL = 16;                            // lists up to here: every thread counts for all entries over its own positions
constexpr int TM_OWN = 4;                               // longer lists: a thread owns up to 4 entries and reads the row from LDS
static_assert(TM_OWN * TM_BLOCK == TM_CAP, "a full list is four entries per thread");

struct RankArgs {
    const float* scores;
    const float* labels;
    const int64_t* index;
    const int64_t* row_ptr;
    double* ndcg;
    double* rr;
    int64_t ld_s, ld_l;
    int32_t n_rows, n_cols, k;
};

struct Row {
    const float* s;
    const float* l;      // NULL: the one positive (l = 1) is at position `tgt`, -1 = none
    int C;               // -1: the row pointers do not describe a row of at most n_cols positions
    int tgt;
};

__device__ inline Row row_of(const RankArgs& A, int r) {
    Row R;
    int64_t base_s, base_l, C;
    if (A.row_ptr) {
        const int64_t b = A.row_ptr[r], e = A.row_ptr[r + 1];
        C = b < 0 ? -1 : e - b;
        base_s = base_l = b;
    } else {
        C = A.n_cols;
        base_s = (int64_t)r * A.ld_s;
        base_l = (int64_t)r * A.ld_l;
    }
    R.C = C < 0 || C > A.n_cols ? -1 : (int)C;
    R.s = A.scores + base_s;
    R.l = A.labels ? A.labels + base_l : nullptr;
    R.tgt = -1;
    if (!A.labels && R.C > 0) {
        const int64_t t = A.index ? A.index[r] : 0;
        if (t >= 0 && t < C) R.tgt = (int)t;
    }
    return R;
}

__device__ inline bool beats(float a, int ja, float b, int jb) { return a > b || (a == b && ja < jb); }

__device__ inline double gain(float l, int rank) { return rank == 0 ? (double)l : (double)l / log2((double)(rank + 1)); }

__device__ inline void write_row(const RankArgs& A, int r, bool nan, double dcg, double idcg, int min_rank) {
    const double q = nan ? (double)NAN : 0.0;
    A.ndcg[r] = nan ? q : (idcg == 0.0 ? 0.0 : dcg / idcg);
    A.rr[r] = nan ? q : (min_rank == INT_MAX ? 0.0 : 1.0 / (double)(1 + min_rank));
}

// ---------------------------------------------------------------------------------------------- rows of at most 64 positions
__global__ void __launch_bounds__(TM_BLOCK) k_rank_wave(RankArgs A) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * TM_WAVES + (threadIdx.x >> 6);
    if (r >= A.n_rows) return;                                                    // wavefront-uniform, like every return below
    const Row R = row_of(A, r);
    if (R.C > 64) return;                                                         // k_rank_block's
    if (R.C < 0) {
        if (lane == 0) write_row(A, r, true, 0.0, 0.0, INT_MAX);
        return;
    }
    const int C = R.C;
    const bool in = lane < C;
    const float s = in ? R.s[lane] : 0.0f;
    const float l = in ? (R.l ? R.l[lane] : (lane == R.tgt ? 1.0f : 0.0f)) : 0.0f;
    const bool nan = __ballot(in && s != s) != 0ull;
    int rank = 0, irank = 0;
    for (int j = 0; j < C; ++j) {
        const float sj = __shfl(s, j), lj = __shfl(l, j);
        rank += beats(sj, j, s, lane);
        irank += beats(lj, j, l, lane);
    }
    const bool pos = in && l > 0.0f;
    const int K = A.k > 0 ? A.k : C;
    double d = pos && rank < K ? gain(l, rank) : 0.0, id = pos && irank < K ? gain(l, irank) : 0.0;
    int mr = pos ? rank : INT_MAX;
    for (int o = 32; o; o >>= 1) {
        d += __shfl_down(d, o);
        id += __shfl_down(id, o);
        mr = min(mr, __shfl_down(mr, o));
    }
    if (lane == 0) write_row(A, r, nan, d, id, mr);
}

// ---------------------------------------------------------------------------------------------- longer rows: a workgroup each
// positions [e0, e1) of the staged tile against the OWN list entries a thread holds.  A position without relevance beats no positive in
// the ideal order, so the second count is taken only where l > 0 (the same for every lane of a wavefront: the reads broadcast).
template <int OWN>
__device__ __forceinline__ void count_owned(const float* ts, const float* tl, int e0, int e1, int j0, const float (&sp)[TM_OWN],
                                            const float (&lq)[TM_OWN], const int (&pp)[TM_OWN], int (&cnt)[TM_OWN], int (&icnt)[TM_OWN]) {
    for (int e = e0; e < e1; ++e) {
        const float s = ts[e], l = tl[e];
        const int j = j0 + e;
#pragma unroll
        for (int i = 0; i < OWN; ++i) cnt[i] += beats(s, j, sp[i], pp[i]);
        if (l > 0.0f) {
#pragma unroll
            for (int i = 0; i < OWN; ++i) icnt[i] += beats(l, j, lq[i], pp[i]);
        }
    }
}

__global__ void __launch_bounds__(TM_BLOCK) k_rank_block(RankArgs A) {
    __shared__ __attribute__((aligned(16))) float ts[TM_TILE];
    __shared__ __attribute__((aligned(16))) float tl[TM_TILE];
    __shared__ float ls[TM_CAP], ll[TM_CAP];
    __shared__ int lp[TM_CAP], lrank[TM_CAP], lirank[TM_CAP];
    __shared__ double wsum[2][TM_WAVES];
    __shared__ int wcount[TM_WAVES], s_min, s_nan;
    const int r = blockIdx.x, k = threadIdx.x, lane = k & 63, wave = k >> 6;
    const Row R = row_of(A, r);
    if (R.C <= 64) return;                                                        // workgroup-uniform: k_rank_wave's (and C = -1)
    const int C = R.C, K = A.k > 0 ? A.k : C;
    const bool vec_s = ((uintptr_t)R.s & 15) == 0, vec_l = R.l && ((uintptr_t)R.l & 15) == 0;
    if (k == 0) {
        s_min = INT_MAX;
        s_nan = 0;
    }
    // positions j .. j + 3 of the row (j a multiple of 4): 16-byte loads where the row's base is aligned and the four lie inside
    auto quad = [&](int j, float (&v)[4], float (&w)[4]) {
        const bool whole = j + 3 < C;
        if (whole && vec_s) {
            const float4 t = *reinterpret_cast<const float4*>(R.s + j);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = j + e < C ? R.s[j + e] : 0.0f;
        }
        if (!R.l) {
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = j + e == R.tgt ? 1.0f : 0.0f;
        } else if (whole && vec_l) {
            const float4 t = *reinterpret_cast<const float4*>(R.l + j);
            w[0] = t.x, w[1] = t.y, w[2] = t.z, w[3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = j + e < C ? R.l[j + e] : 0.0f;
        }
    };

    // where the walk that fills the list stands: the tile at `cj` is the next to look at, `seen` positives lie in front of it
    int cj = 0, seen = 0;
    double dcg = 0.0, idcg = 0.0;
    for (int pass = 0;; ++pass) {
        // ---- the list: positives number [lo, lo + TM_CAP) of the row, in position order
        const int lo = pass * TM_CAP;
        int L = 0;
        if (!R.l) {
            if (R.tgt >= 0) {
                L = 1;
                if (k == 0) ls[0] = R.s[R.tgt], ll[0] = 1.0f, lp[0] = R.tgt;
            }
        } else {
            while (cj < C) {
                float v[4], w[4];
                const int j = cj + 4 * k;
                quad(j, v, w);
                int mine = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) mine += w[e] > 0.0f;                  // (positions past the row's end were read as 0)
                int inc = mine;
                for (int o = 1; o < 64; o <<= 1) {
                    const int up = __shfl_up(inc, o);
                    if (lane >= o) inc += up;
                }
                if (lane == 63) wcount[wave] = inc;
                __syncthreads();
                int ord = seen + inc - mine, total = 0;
                for (int q = 0; q < TM_WAVES; ++q) {
                    if (q < wave) ord += wcount[q];
                    total += wcount[q];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (w[e] > 0.0f) {
                        const int slot = ord - lo;
                        if (slot >= 0 && slot < TM_CAP) ls[slot] = v[e], ll[slot] = w[e], lp[slot] = j + e;
                        ++ord;
                    }
                }
                __syncthreads();                                                  // wcount is written again by the next tile
                const int after = seen + total;
                if (after > lo + TM_CAP) {                                        // the rest of this tile belongs to the next pass
                    L = TM_CAP;
                    break;
                }
                seen = after;
                cj += TM_TILE;
                L = max(after - lo, 0);
                if (L == TM_CAP) break;
            }
        }
        if (pass > 0 && L == 0) break;                                            // (pass 0 streams the row even so: it looks for NaN)
        for (int i = k; i < L; i += TM_BLOCK) lrank[i] = 0, lirank[i] = 0;
        __syncthreads();

        // ---- both counts of every entry: one stream of the row
        if (L <= TM_SMALL) {
            // few entries: every thread counts for all of them over its own positions, straight from memory
            int cnt[TM_SMALL], icnt[TM_SMALL];
#pragma unroll
            for (int i = 0; i < TM_SMALL; ++i) cnt[i] = icnt[i] = 0;
            bool nan = false;
            for (int j0 = 0; j0 < C; j0 += TM_TILE) {
                const int j = j0 + 4 * k;
                if (j >= C) break;
                float v[4], w[4];
                quad(j, v, w);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (j + e >= C) continue;
                    nan |= v[e] != v[e];
#pragma unroll
                    for (int i = 0; i < TM_SMALL; ++i) {
                        if (i < L) cnt[i] += beats(v[e], j + e, ls[i], lp[i]);
                    }
                    if (w[e] > 0.0f) {                                            // a position without relevance beats no positive
#pragma unroll
                        for (int i = 0; i < TM_SMALL; ++i) {
                            if (i < L) icnt[i] += beats(w[e], j + e, ll[i], lp[i]);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < TM_SMALL; ++i) {
                if (i < L) {                                                      // workgroup-uniform
                    int a = cnt[i], b = icnt[i];
                    for (int o = 32; o; o >>= 1) a += __shfl_down(a, o), b += __shfl_down(b, o);
                    if (lane == 0) atomicAdd(&lrank[i], a), atomicAdd(&lirank[i], b);
                }
            }
            if (nan) s_nan = 1;
        } else {
            // the row goes through LDS a tile at a time; `parts` groups of threads share the entries and split each tile between them
            const int parts = L <= TM_BLOCK ? 4 : L <= 2 * TM_BLOCK ? 2 : 1, width = TM_BLOCK / parts;
            const int slot = k % width, part = k / width, per = TM_TILE / parts, own = (L + width - 1) / width;
            float sp[TM_OWN], lq[TM_OWN];
            int pp[TM_OWN], cnt[TM_OWN], icnt[TM_OWN];
#pragma unroll
            for (int i = 0; i < TM_OWN; ++i) {
                const int at = slot + i * width;
                const bool have = at < L;
                sp[i] = have ? ls[at] : 0.0f, lq[i] = have ? ll[at] : 0.0f, pp[i] = have ? lp[at] : -1;
                cnt[i] = icnt[i] = 0;
            }
            bool nan = false;
            for (int j0 = 0; j0 < C; j0 += TM_TILE) {
                float v[4], w[4];
                quad(j0 + 4 * k, v, w);
#pragma unroll
                for (int e = 0; e < 4; ++e) nan |= v[e] != v[e];                  // (positions past the end were read as 0)
                *reinterpret_cast<float4*>(&ts[4 * k]) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4*>(&tl[4 * k]) = make_float4(w[0], w[1], w[2], w[3]);
                __syncthreads();
                const int e0 = part * per, e1 = min(e0 + per, C - j0);           // wavefront-uniform bounds: the reads broadcast
                switch (own) {
                    case 1: count_owned<1>(ts, tl, e0, e1, j0, sp, lq, pp, cnt, icnt); break;
                    case 2: count_owned<2>(ts, tl, e0, e1, j0, sp, lq, pp, cnt, icnt); break;
                    case 3: count_owned<3>(ts, tl, e0, e1, j0, sp, lq, pp, cnt, icnt); break;
                    default: count_owned<4>(ts, tl, e0, e1, j0, sp, lq, pp, cnt, icnt); break;
                }
                __syncthreads();
            }
#pragma unroll
            for (int i = 0; i < TM_OWN; ++i) {
                const int at = slot + i * width;
                if (at < L) atomicAdd(&lrank[at], cnt[i]), atomicAdd(&lirank[at], icnt[i]);
            }
            if (nan) s_nan = 1;
        }
        __syncthreads();

        // ---- the terms of this pass, in list order
        double d = 0.0, id = 0.0;
        int mr = INT_MAX;
        for (int i = k; i < L; i += TM_BLOCK) {
            const int rank = lrank[i], irank = lirank[i];
            const float l = ll[i];
            if (rank < K) d += gain(l, rank);
            if (irank < K) id += gain(l, irank);
            mr = min(mr, rank);
        }
        for (int o = 32; o; o >>= 1) {
            d += __shfl_down(d, o);
            id += __shfl_down(id, o);
            mr = min(mr, __shfl_down(mr, o));
        }
        if (lane == 0) {
            wsum[0][wave] = d, wsum[1][wave] = id;
            if (mr != INT_MAX) atomicMin(&s_min, mr);
        }
        __syncthreads();
        for (int q = 0; q < TM_WAVES; ++q) dcg += wsum[0][q], idcg += wsum[1][q];   // every thread, the same order
        __syncthreads();                                                          // the list and wsum are written again by the next pass
        if (L < TM_CAP) break;
    }
    if (k == 0) write_row(A, r, s_nan != 0, dcg, idcg, s_min);
}

// ---------------------------------------------------------------------------------------------- the pair-ranking loss
struct NllArgs {
    const float* scores;
    const int64_t* row_ptr;
    float* loss;
    float* lse;                  // [n_seg][2]: max, log(sum exp(x - max))
    const float* lse_in;
    const float* grad_loss;
    float* grad_scores;
    int32_t n_seg, max_len;
};

// the length of segment r: 2 .. max_len, or 0 = the row pointers do not describe such a segment (1 = a single entry)
__device__ inline int segment_of(const NllArgs& A, int r, int64_t& beg) {
    const int64_t b = A.row_ptr[r], len = A.row_ptr[r + 1] - b;
    beg = b;
    return b < 0 || len < 1 || len > A.max_len ? 0 : (int)len;
}

__device__ inline float ln_len(int len) { return (float)log((double)len); }       // the fp32 value nearest to ln(len)

__device__ inline float wave_max(float x) {
    for (int o = 32; o; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
    return x;
}

__device__ inline float wave_sum(float x) {
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

template <bool BWD>
__global__ void __launch_bounds__(TM_BLOCK) k_nll_wave(NllArgs A) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * TM_WAVES + (threadIdx.x >> 6);
    if (r >= A.n_seg) return;
    int64_t beg;
    const int len = segment_of(A, r, beg);
    if (len > 64) return;                                                         // k_nll_block's
    if (len < 2) {                                                                // no loss is defined: NaN, never a stale value
        if (BWD) {
            if (len == 1 && lane == 0) A.grad_scores[beg] = NAN;
        } else if (lane == 0) {
            A.loss[r] = A.lse[2 * r] = A.lse[2 * r + 1] = NAN;
        }
        return;
    }
    const bool in = lane < len;
    const float x = in ? A.scores[beg + lane] : -INFINITY;
    const float scale = ln_len(len);
    if (BWD) {
        const float m = A.lse_in[2 * r], ls = A.lse_in[2 * r + 1], g = A.grad_loss[r];
        if (in) A.grad_scores[beg + lane] = g * (expf((x - m) - ls) - (lane == 0 ? 1.0f : 0.0f)) / scale;
    } else {
        const float m = wave_max(x);                                              // (a NaN entry still reaches the sum)
        const float sum = wave_sum(in ? expf(x - m) : 0.0f), ls = logf(sum);
        const float x0 = __shfl(x, 0);
        if (lane == 0) {
            A.loss[r] = (ls - (x0 - m)) / scale;
            A.lse[2 * r] = m, A.lse[2 * r + 1] = ls;
        }
    }
}

template <bool BWD>
__global__ void __launch_bounds__(TM_BLOCK) k_nll_block(NllArgs A) {
    __shared__ float part[TM_WAVES];
    const int r = blockIdx.x, k = threadIdx.x, lane = k & 63, wave = k >> 6;
    int64_t beg;
    const int len = segment_of(A, r, beg);
    if (len <= 64) return;                                                        // workgroup-uniform: k_nll_wave's
    const float* x = A.scores + beg;
    const float scale = ln_len(len);
    if (BWD) {
        const float m = A.lse_in[2 * r], ls = A.lse_in[2 * r + 1], g = A.grad_loss[r];
        for (int j = k; j < len; j += TM_BLOCK) A.grad_scores[beg + j] = g * (expf((x[j] - m) - ls) - (j == 0 ? 1.0f : 0.0f)) / scale;
        return;
    }
    float m = -INFINITY;
    for (int j = k; j < len; j += TM_BLOCK) m = fmaxf(m, x[j]);
    m = wave_max(m);
    if (lane == 0) part[wave] = m;
    __syncthreads();
    m = part[0];
    for (int q = 1; q < TM_WAVES; ++q) m = fmaxf(m, part[q]);
    __syncthreads();
    float sum = 0.0f;
    for (int j = k; j < len; j += TM_BLOCK) sum += expf(x[j] - m);
    sum = wave_sum(sum);
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (k == 0) {
        sum = part[0];
        for (int q = 1; q < TM_WAVES; ++q) sum += part[q];
        const float ls = logf(sum);
        A.loss[r] = (ls - (x[0] - m)) / scale;
        A.lse[2 * r] = m, A.lse[2 * r + 1] = ls;
    }
}

int nll_args_ok(const float* scores, const int64_t* row_ptr, int32_t n_seg, int32_t max_len) {
    if (n_seg < 0 || max_len < 0) return HGT_ERR_INVALID_ARG;
    if (n_seg == 0) return HGT_OK;
    if (max_len < 2 || !scores || !row_ptr) return HGT_ERR_INVALID_ARG;
    return HGT_OK;
}

}  // namespace

extern "C" int hgt_rank_metrics(const float* scores, const float* labels, const int64_t* index, const int64_t* row_ptr, int32_t n_rows,
                                int32_t n_cols, int64_t ld_scores, int64_t ld_labels, int32_t k, double* ndcg_out, double* rr_out,
                                void* stream) {
    if (n_rows < 0 || n_cols < 0 || k < 0 || (labels && index)) return HGT_ERR_INVALID_ARG;
    if (n_rows == 0) return HGT_OK;
    if (!ndcg_out || !rr_out) return HGT_ERR_INVALID_ARG;
    if (n_cols > INT_MAX - TM_TILE) return HGT_ERR_UNSUPPORTED;                    // positions are 32-bit, a tile past the end included
    if (n_cols > 0 && !scores) return HGT_ERR_INVALID_ARG;
    if (!row_ptr && (ld_scores < n_cols || (labels && ld_labels < n_cols))) return HGT_ERR_INVALID_ARG;
    RankArgs A;
    A.scores = scores; A.labels = labels; A.index = index; A.row_ptr = row_ptr; A.ndcg = ndcg_out; A.rr = rr_out;
    A.ld_s = ld_scores; A.ld_l = ld_labels; A.n_rows = n_rows; A.n_cols = n_cols; A.k = k;
    if (row_ptr || n_cols <= 64) {
        k_rank_wave<<<(unsigned)((n_rows + TM_WAVES - 1) / TM_WAVES), TM_BLOCK, 0, (hipStream_t)stream>>>(A);
        HGT_CHECK_LAUNCH();
    }
    if (n_cols > 64) {
        k_rank_block<<<(unsigned)n_rows, TM_BLOCK, 0, (hipStream_t)stream>>>(A);
        HGT_CHECK_LAUNCH();
    }
    return HGT_OK;
}

extern "C" int hgt_segment_first_nll(const float* scores, const int64_t* row_ptr, int32_t n_seg, int32_t max_len, float* loss_out,
                                     float* lse_out, void* stream) {
    const int rc = nll_args_ok(scores, row_ptr, n_seg, max_len);
    if (rc != HGT_OK || n_seg == 0) return rc;
    if (!loss_out || !lse_out) return HGT_ERR_INVALID_ARG;
    NllArgs A = {};
    A.scores = scores; A.row_ptr = row_ptr; A.loss = loss_out; A.lse = lse_out; A.n_seg = n_seg; A.max_len = max_len;
    k_nll_wave<false><<<(unsigned)((n_seg + TM_WAVES - 1) / TM_WAVES), TM_BLOCK, 0, (hipStream_t)stream>>>(A);
    HGT_CHECK_LAUNCH();
    if (max_len > 64) {
        k_nll_block<false><<<(unsigned)n_seg, TM_BLOCK, 0, (hipStream_t)stream>>>(A);
        HGT_CHECK_LAUNCH();
    }
    return HGT_OK;
}

extern "C" int hgt_segment_first_nll_bwd(const float* scores, const int64_t* row_ptr, int32_t n_seg, int32_t max_len, const float* lse,
                                         const float* grad_loss, float* grad_scores, void* stream) {
    const int rc = nll_args_ok(scores, row_ptr, n_seg, max_len);
    if (rc != HGT_OK || n_seg == 0) return rc;
    if (!lse || !grad_loss || !grad_scores) return HGT_ERR_INVALID_ARG;
    NllArgs A = {};
    A.scores = scores; A.row_ptr = row_ptr; A.lse_in = lse; A.grad_loss = grad_loss; A.grad_scores = grad_scores;
    A.n_seg = n_seg; A.max_len = max_len;
    k_nll_wave<true><<<(unsigned)((n_seg + TM_WAVES - 1) / TM_WAVES), TM_BLOCK, 0, (hipStream_t)stream>>>(A);
    HGT_CHECK_LAUNCH();
    if (max_len > 64) {
        k_nll_block<true><<<(unsigned)n_seg, TM_BLOCK, 0, (hipStream_t)stream>>>(A);
        HGT_CHECK_LAUNCH();
    }
    return HGT_OK;
}
