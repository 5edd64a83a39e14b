// Task labels on the device (gfx950): for n nodes of a triple's target type, the classes of their neighbours in the resident CSR of
// the device sampler (hgt_sampler.hip) -- what the reference's training scripts build in Python between sample_subgraph and the
// model (OAG/train_paper_field.py:133-137: a distribution over the fields of a paper; train_paper_venue.py:134: the index of its
// venue), without a host copy of an id.
//
//   row r, v = ids[r]   a neighbour at position p of v's row qualifies iff col_of[src[p]] >= 0 (and below n_cols) and, with a window,
//                       time[p] != HGT_SAMPLER_TIME_NONE and t_min <= time[p] <= t_max
//   C                   the set of distinct columns of the qualifying neighbours
//   dist[r, c]          1.0f / (float)|C| for c in C, 0 for every other c < n_cols (the whole row is written; the padding is not)
//   index[r]            the column of the first qualifying neighbour in adjacency order, -1 without one
//   count[r]            |C|
//   columns[r, i]       hgt_sampler_label_columns: the i-th smallest column of C for i < min(|C|, width), -1 behind it -- the same set
//                       as a list, for hgt_class_loss, in place of a dense row that holds a handful of non-zeros
//
// One workgroup per row.  C is a bitmap in LDS (integer atomicOr: the same bits whatever the order), LABEL_CHUNK columns a pass; the
// first qualifying position is an integer atomicMin.  The count is known before a value is written, so a row is written once, each
// element by one thread: no float atomics, and nothing depends on the launch geometry.  Compiled without fast-math like the rest of
// the library: 1.0f / count is the IEEE quotient.  The list form walks the same bitmap: a thread owns LABEL_WORDS / LABEL_BLOCK
// consecutive words, a prefix sum of their popcounts over the workgroup gives the place of its first column, and the columns of a
// chunk follow those of the chunks in front of it -- ascending, each written by one thread.
#include "hgt_common.h"

namespace {

constexpr int LABEL_BLOCK = 256;
constexpr int LABEL_WORDS = 4096;                       // 16 KB of LDS
constexpr int LABEL_CHUNK = LABEL_WORDS * 32;           // columns a pass of the bitmap covers
constexpr int LABEL_OWN = LABEL_WORDS / LABEL_BLOCK;    // list form: consecutive words a thread owns

struct LabelArgs {
    const int32_t* indptr;
    const int32_t* src;
    const int32_t* time;
    const int32_t* ids;
    const int32_t* col_of;
    float* dist;
    int32_t* index;
    int32_t* count;
    int32_t* columns;
    int64_t ld;
    int32_t width;
    int32_t n_tgt, n_src, n, n_cols, has_window, t_min, t_max;
};

template <bool LIST>
__global__ void __launch_bounds__(LABEL_BLOCK) k_labels(LabelArgs A) {
    __shared__ uint32_t bits[LABEL_WORDS];
    __shared__ int first, total, wtot[LABEL_BLOCK / 64];
    const int r = blockIdx.x, k = threadIdx.x;
    if (r >= A.n) return;                                                         // workgroup-uniform
    const int v = A.ids[r];
    int beg = 0, deg = 0;
    if ((unsigned)v < (unsigned)A.n_tgt && A.n_src > 0) {
        beg = A.indptr[v];
        deg = A.indptr[v + 1] - beg;
        if (deg < 0) deg = 0;
    }
    if (k == 0) {
        first = deg;
        total = 0;
    }
    // the column of the neighbour at position p, -1: it does not qualify
    auto column = [&](int p) -> int {
        const int s = A.src[beg + p];
        if ((unsigned)s >= (unsigned)A.n_src) return -1;
        if (A.has_window) {
            const int32_t tm = A.time[beg + p];
            if (tm == HGT_SAMPLER_TIME_NONE || tm < A.t_min || tm > A.t_max) return -1;
        }
        const int c = A.col_of[s];
        return (unsigned)c < (unsigned)A.n_cols ? c : -1;
    };
    // the bitmap of the columns [c0, c0 + LABEL_CHUNK) of C; every thread calls
    auto mark = [&](int c0, int words, bool want_first) {
        for (int w = k; w < words; w += LABEL_BLOCK) bits[w] = 0u;
        __syncthreads();
        for (int p = k; p < deg; p += LABEL_BLOCK) {
            const int c = column(p);
            if (c < 0) continue;
            if (want_first) atomicMin(&first, p);
            const int rel = c - c0;
            if (rel >= 0 && rel < LABEL_CHUNK) atomicOr(&bits[rel >> 5], 1u << (rel & 31));
        }
        __syncthreads();
    };
    auto words_of = [&](int c0) { return (min(A.n_cols - c0, LABEL_CHUNK) + 31) >> 5; };
    const bool one_pass = A.n_cols <= LABEL_CHUNK;
    __syncthreads();
    if constexpr (LIST) {
        int32_t* out = A.columns + (int64_t)r * A.width;
        const int lane = k & 63, wave = k >> 6;
        int seen = 0;                                                             // classes in the chunks in front of this one
        for (int c0 = 0; c0 < A.n_cols; c0 += LABEL_CHUNK) {
            const int words = words_of(c0);
            mark(c0, words, false);
            int mine = 0;
            for (int i = 0; i < LABEL_OWN; ++i) {
                const int w = k * LABEL_OWN + i;
                if (w < words) mine += __popc(bits[w]);
            }
            int inc = mine;
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(inc, o);
                if (lane >= o) inc += up;
            }
            if (lane == 63) wtot[wave] = inc;
            __syncthreads();
            int at = seen + inc - mine;
            for (int q = 0; q < LABEL_BLOCK / 64; ++q) {
                if (q < wave) at += wtot[q];
                seen += wtot[q];
            }
            for (int i = 0; i < LABEL_OWN; ++i) {
                const int w = k * LABEL_OWN + i;
                uint32_t word = w < words ? bits[w] : 0u;
                while (word) {
                    if (at < A.width) out[at] = c0 + w * 32 + (__ffs(word) - 1);
                    ++at;
                    word &= word - 1u;
                }
            }
            __syncthreads();                                                      // bits and wtot are written again by the next chunk
        }
        for (int i = seen + k; i < A.width; i += LABEL_BLOCK) out[i] = -1;
        if (k == 0 && A.count) A.count[r] = seen;
        return;
    }
    for (int c0 = 0; c0 < A.n_cols; c0 += LABEL_CHUNK) {
        const int words = words_of(c0);
        mark(c0, words, c0 == 0);
        int c = 0;
        for (int w = k; w < words; w += LABEL_BLOCK) c += __popc(bits[w]);
        if (c) atomicAdd(&total, c);
        __syncthreads();
    }
    const int n_classes = total, p_first = first;
    if (k == 0) {
        if (A.index) A.index[r] = p_first < deg ? column(p_first) : -1;
        if (A.count) A.count[r] = n_classes;
    }
    if (!A.dist) return;
    const float value = n_classes > 0 ? 1.0f / (float)n_classes : 0.0f;
    float* row = A.dist + (int64_t)r * A.ld;
    for (int c0 = 0; c0 < A.n_cols; c0 += LABEL_CHUNK) {
        if (!one_pass) mark(c0, words_of(c0), false);                             // one pass: the bitmap of the count loop is still there
        const int cols = min(A.n_cols - c0, LABEL_CHUNK);
        for (int c = k; c < cols; c += LABEL_BLOCK) row[c0 + c] = (bits[c >> 5] >> (c & 31)) & 1u ? value : 0.0f;
        __syncthreads();
    }
}

// the checks and the input half of the arguments that both entry points share (n == 0: HGT_OK with nothing filled in)
int label_args(const hgt_sampler_triple* triple_host, int32_t n_tgt_nodes, int32_t n_src_nodes, const int32_t* ids, int32_t n,
               const int32_t* col_of, int32_t n_cols, int32_t has_window, int32_t t_min, int32_t t_max, LabelArgs& A) {
    if (n < 0 || n_tgt_nodes < 0 || n_src_nodes < 0 || n_cols < 0) return HGT_ERR_INVALID_ARG;
    if (has_window && t_min > t_max) return HGT_ERR_INVALID_ARG;
    if (n == 0) return HGT_OK;
    if (!triple_host || !ids) return HGT_ERR_INVALID_ARG;
    const hgt_sampler_triple& tr = *triple_host;
    if (!tr.indptr) return HGT_ERR_INVALID_ARG;                                   // [n_tgt_nodes + 1] entries even without a node
    if (n_tgt_nodes > 0 && n_src_nodes > 0 && (!tr.src || !col_of || (has_window && !tr.time))) return HGT_ERR_INVALID_ARG;
    A.indptr = tr.indptr; A.src = tr.src; A.time = tr.time; A.ids = ids; A.col_of = col_of;
    A.n_tgt = n_tgt_nodes; A.n_src = n_src_nodes; A.n = n; A.n_cols = n_cols;
    A.has_window = has_window != 0; A.t_min = t_min; A.t_max = t_max;
    return HGT_OK;
}

}  // namespace

extern "C" int hgt_sampler_labels(const hgt_sampler_triple* triple_host, int32_t n_tgt_nodes, int32_t n_src_nodes, const int32_t* ids, int32_t n,
                                  const int32_t* col_of, int32_t n_cols, int32_t has_window, int32_t t_min, int32_t t_max, float* dist_out,
                                  int64_t ld, int32_t* index_out, int32_t* count_out, void* stream) {
    if (dist_out && ld < n_cols) return HGT_ERR_INVALID_ARG;
    LabelArgs A;
    const int rc = label_args(triple_host, n_tgt_nodes, n_src_nodes, ids, n, col_of, n_cols, has_window, t_min, t_max, A);
    if (rc != HGT_OK || n == 0) return rc;
    A.dist = dist_out; A.index = index_out; A.count = count_out; A.ld = ld;
    A.columns = nullptr; A.width = 0;
    k_labels<false><<<(unsigned)n, LABEL_BLOCK, 0, (hipStream_t)stream>>>(A);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_sampler_label_columns(const hgt_sampler_triple* triple_host, int32_t n_tgt_nodes, int32_t n_src_nodes, const int32_t* ids,
                                         int32_t n, const int32_t* col_of, int32_t n_cols, int32_t has_window, int32_t t_min, int32_t t_max,
                                         int32_t* columns_out, int32_t width, int32_t* count_out, void* stream) {
    LabelArgs A;
    const int rc = label_args(triple_host, n_tgt_nodes, n_src_nodes, ids, n, col_of, n_cols, has_window, t_min, t_max, A);
    if (rc != HGT_OK) return rc;
    if (width < 1) return HGT_ERR_INVALID_ARG;
    if (n == 0) return HGT_OK;
    if (!columns_out) return HGT_ERR_INVALID_ARG;
    A.dist = nullptr; A.index = nullptr; A.count = count_out; A.ld = 0;
    A.columns = columns_out; A.width = width;
    k_labels<true><<<(unsigned)n, LABEL_BLOCK, 0, (hipStream_t)stream>>>(A);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}
