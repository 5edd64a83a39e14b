// Voted evaluation of the node-property task on the device (gfx950): what the reference's ogbn-mag scripts do with the Classifier's
// output besides the loss -- the per-split accuracies of a training step (ogbn-mag/train_ogbn_mag.py:165-191: argmax of the rows of a
// split against y) and the vote of eval_ogbn_mag.py:128-191 (every test paper owns C sums, each sampled sub-graph adds the
// log-probabilities of the test papers it holds, the answer is the argmax of the sums).
//
//   hgt_class_predict   pred[r] = np.argmax of row r: the lowest position among the maxima, a NaN beats every number (the first NaN
//                       wins), -inf and +inf are ordinary values.  With labels, a row is scored in split s iff label >= 0 and
//                       0 <= split < n_splits: counts[2 s] += 1, counts[2 s + 1] += (pred == label).  Labels and splits are per-row
//                       arrays, or resident tables read at ids[r] (an id outside the table: not scored, nothing read).
//   hgt_vote_add        votes[slot_of[ids[r]]][j] += (x_rj - m) - ls, count[slot] += 1: the float32 log-softmax of hgt_class_loss
//                       (hgt_row_common.h forms m and ls for both), added in place.  One launch per piece; inside a piece the
//                       slotted ids are distinct by contract, so a slot has one writer per launch and stream order fixes the order
//                       of the additions across pieces: no atomics, the same bits every time.
//
// Rows of at most HGT_CLASS_LOSS_WAVE_COLS columns take a wavefront each, longer ones a workgroup each.  Position j of a row always
// belongs to the same thread -- 16-byte loads where the row's base is aligned, four scalar loads where it is not.  The prediction is
// a (value, position) pair under a total order, joined by a shuffle tree and then through LDS across the wavefronts: the result is the
// same whatever the order of the joins.  The counts are integers: a workgroup sums its rows in LDS and adds the non-zero sums to the
// (zeroed) output with integer atomics, whose total does not depend on their order.  No float atomics.
#include <limits.h>
#include <math.h>

#include "hgt_common.h"
#include "hgt_row_common.h"

namespace {

struct PredictArgs {
    const float* x;
    const int64_t* ids;
    const int64_t* label;
    const int32_t* split;
    int64_t* pred;
    int32_t* counts;
    int64_t ld, n_table;
    int32_t n_rows, n_cols, n_splits, rows_per_group;
};

struct VoteArgs {
    const float* x;
    const int64_t* ids;
    const int32_t* slot_of;
    float* votes;
    int32_t* count;
    int64_t ld, ld_votes, n_nodes;
    int32_t row_begin, row_end, n_cols, n_slots;
};

struct Scratch {
    float f[CL_WAVES];
    int p[CL_WAVES];
    int counts[2 * HGT_PREDICT_MAX_SPLITS];
};

// np.argmax's order: does (a, pa) come before (b, pb)?  A NaN before every number, then the larger value, then the lower position
__device__ __forceinline__ bool before(float a, int pa, float b, int pb) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && nb ? pa < pb : na;
    return a != b ? a > b : pa < pb;
}

template <int T>
__device__ __forceinline__ int group_argmax(float v, int p, Scratch& S) {
    for (int o = 32; o; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int op = __shfl_xor(p, o);
        if (before(ov, op, v, p)) v = ov, p = op;
    }
    if (T == 64) return p;
    if ((threadIdx.x & 63) == 0) S.f[threadIdx.x >> 6] = v, S.p[threadIdx.x >> 6] = p;
    __syncthreads();
    v = S.f[0], p = S.p[0];
    for (int q = 1; q < CL_WAVES; ++q) {
        if (before(S.f[q], S.p[q], v, p)) v = S.f[q], p = S.p[q];
    }
    __syncthreads();
    return p;
}

// T = 64: a wavefront per row, T = CL_BLOCK: a workgroup per row; a group takes rows_per_group consecutive rows
template <int T>
__global__ void __launch_bounds__(CL_BLOCK) k_class_predict(PredictArgs A) {
    __shared__ Scratch S;
    const int k = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int64_t group = T == 64 ? (int64_t)blockIdx.x * CL_WAVES + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    const int C = A.n_cols;
    if (A.counts) {
        if (threadIdx.x < 2 * HGT_PREDICT_MAX_SPLITS) S.counts[threadIdx.x] = 0;
        __syncthreads();
    }
    const int64_t first = group * A.rows_per_group;
    for (int64_t r = first; r < first + A.rows_per_group && r < A.n_rows; ++r) {   // uniform over the T threads
        const float* x = A.x + r * A.ld;
        const bool vec = ((uintptr_t)x & 15) == 0;
        float best = -INFINITY;
        int pos = INT_MAX;                                                        // (loses against every position of the row)
        for (int j = 4 * k; j < C; j += 4 * T) {
            float v[4];
            load4(x, j, C, vec, -INFINITY, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (j + e < C && before(v[e], j + e, best, pos)) best = v[e], pos = j + e;
            }
        }
        pos = group_argmax<T>(best, pos, S);
        if (k != 0) continue;
        if (A.pred) A.pred[r] = pos;
        if (!A.counts) continue;
        int64_t at = r;
        if (A.ids) {
            at = A.ids[r];
            if (at < 0 || at >= A.n_table) continue;
        }
        const int64_t y = A.label[at];
        const int32_t s = A.split ? A.split[at] : 0;
        if (y < 0 || s < 0 || s >= A.n_splits) continue;
        atomicAdd(&S.counts[2 * s], 1);
        if (y == pos) atomicAdd(&S.counts[2 * s + 1], 1);
    }
    if (A.counts) {
        __syncthreads();
        if ((int)threadIdx.x < 2 * A.n_splits && S.counts[threadIdx.x]) atomicAdd(&A.counts[threadIdx.x], S.counts[threadIdx.x]);
    }
}

// one piece: rows row_begin .. row_end.  T = 64: a wavefront per row, four rows a workgroup;  T = CL_BLOCK: a workgroup per row
template <int T>
__global__ void __launch_bounds__(CL_BLOCK) k_vote_add(VoteArgs A) {
    __shared__ Scratch S;
    const int k = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int64_t r = A.row_begin + (T == 64 ? (int64_t)blockIdx.x * CL_WAVES + (threadIdx.x >> 6) : (int64_t)blockIdx.x);
    if (r >= A.row_end) return;                                                   // uniform over the T threads, like every branch below
    const int64_t id = A.ids[r];
    if (id < 0 || id >= A.n_nodes) return;
    const int32_t slot = A.slot_of[id];
    if (slot < 0 || slot >= A.n_slots) return;
    const int C = A.n_cols;
    const float* x = A.x + r * A.ld;
    float* out = A.votes + (int64_t)slot * A.ld_votes;
    const bool vec = ((uintptr_t)x & 15) == 0, vec_o = ((uintptr_t)out & 15) == 0;
    float own[4], m, ls;
    row_lse<T>(x, C, vec, k, own, S, m, ls);
    for (int j = 4 * k; j < C; j += 4 * T) {
        float v[4], o[4];
        if (T == 64) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = own[e];
        } else {
            load4(x, j, C, vec, 0.0f, v);
        }
        load4(out, j, C, vec_o, 0.0f, o);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += (v[e] - m) - ls;
        if (vec_o && j + 3 < C) {
            *reinterpret_cast<float4*>(out + j) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (j + e < C) out[j + e] = o[e];
            }
        }
    }
    if (k == 0) A.count[slot] += 1;
}

}  // namespace

extern "C" int hgt_class_predict(const float* scores, int64_t ld, int32_t n_rows, int32_t n_cols, const int64_t* ids, int64_t n_table,
                                 const int64_t* label, const int32_t* split, int32_t n_splits, int64_t* pred_out, int32_t* counts_out,
                                 void* stream) {
    if (n_rows < 0 || n_cols < 0 || n_table < 0 || ld < n_cols) return HGT_ERR_INVALID_ARG;
    if (!pred_out && !counts_out) return HGT_ERR_INVALID_ARG;
    if ((counts_out || split) && !label) return HGT_ERR_INVALID_ARG;
    if (n_splits < 1 || n_splits > (split ? HGT_PREDICT_MAX_SPLITS : 1)) return HGT_ERR_INVALID_ARG;
    if (n_rows > 0) {
        if (n_cols < 1) return HGT_ERR_INVALID_ARG;
        if (n_cols > INT_MAX - 4 * CL_BLOCK) return HGT_ERR_UNSUPPORTED;            // positions are 32-bit, a step past the end included
        if (!scores) return HGT_ERR_INVALID_ARG;
    }
    if (counts_out && hipMemsetAsync(counts_out, 0, 2 * sizeof(int32_t) * n_splits, (hipStream_t)stream) != hipSuccess) return HGT_ERR_LAUNCH;
    if (n_rows == 0) return HGT_OK;
    PredictArgs A = {};
    A.x = scores; A.ids = ids; A.label = label; A.split = split; A.pred = pred_out; A.counts = counts_out;
    A.ld = ld; A.n_table = ids ? n_table : n_rows; A.n_rows = n_rows; A.n_cols = n_cols; A.n_splits = n_splits;
    A.rows_per_group = n_rows >= 8192 ? 8 : n_rows >= 1024 ? n_rows / 1024 : 1;  // fewer count atomics on a long batch; integers either way
    const int64_t groups = ((int64_t)n_rows + A.rows_per_group - 1) / A.rows_per_group;
    if (n_cols <= HGT_CLASS_LOSS_WAVE_COLS)
        k_class_predict<64><<<(unsigned)((groups + CL_WAVES - 1) / CL_WAVES), CL_BLOCK, 0, (hipStream_t)stream>>>(A);
    else
        k_class_predict<CL_BLOCK><<<(unsigned)groups, CL_BLOCK, 0, (hipStream_t)stream>>>(A);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_vote_add(const float* logits, int64_t ld, int32_t n_cols, const int64_t* ids, const int32_t* piece_ptr_host,
                            int32_t n_pieces, const int32_t* slot_of, int64_t n_nodes, float* votes, int64_t ld_votes, int32_t* count,
                            int32_t n_slots, void* stream) {
    if (n_pieces < 0 || n_cols < 0 || n_nodes < 0 || n_slots < 0 || ld < n_cols || ld_votes < n_cols) return HGT_ERR_INVALID_ARG;
    if (n_pieces == 0) return HGT_OK;
    if (!piece_ptr_host || piece_ptr_host[0] < 0) return HGT_ERR_INVALID_ARG;
    for (int32_t b = 0; b < n_pieces; ++b) {
        if (piece_ptr_host[b + 1] < piece_ptr_host[b]) return HGT_ERR_INVALID_ARG;
    }
    if (piece_ptr_host[n_pieces] == piece_ptr_host[0]) return HGT_OK;
    if (n_cols < 1) return HGT_ERR_INVALID_ARG;
    if (n_cols > INT_MAX - 4 * CL_BLOCK) return HGT_ERR_UNSUPPORTED;
    if (!logits || !ids || !slot_of || !votes || !count) return HGT_ERR_INVALID_ARG;
    if (n_nodes == 0 || n_slots == 0) return HGT_OK;                               // no row has a slot
    VoteArgs A = {};
    A.x = logits; A.ids = ids; A.slot_of = slot_of; A.votes = votes; A.count = count;
    A.ld = ld; A.ld_votes = ld_votes; A.n_nodes = n_nodes; A.n_cols = n_cols; A.n_slots = n_slots;
    for (int32_t b = 0; b < n_pieces; ++b) {
        A.row_begin = piece_ptr_host[b], A.row_end = piece_ptr_host[b + 1];
        const int32_t n = A.row_end - A.row_begin;
        if (n == 0) continue;
        if (n_cols <= HGT_CLASS_LOSS_WAVE_COLS)
            k_vote_add<64><<<(unsigned)((n + CL_WAVES - 1) / CL_WAVES), CL_BLOCK, 0, (hipStream_t)stream>>>(A);
        else
            k_vote_add<CL_BLOCK><<<(unsigned)n, CL_BLOCK, 0, (hipStream_t)stream>>>(A);
        HGT_CHECK_LAUNCH();
    }
    return HGT_OK;
}
