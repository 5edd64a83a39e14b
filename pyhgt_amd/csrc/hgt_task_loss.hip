// Classification losses of a task batch on the device (gfx950): what the reference's paper-venue, ogbn-mag and paper-field scripts do
// with the Classifier's output -- log_softmax, then nll_loss (OAG/train_paper_venue.py:86, ogbn-mag/train_ogbn_mag.py:116) or
// KLDivLoss(reduction='batchmean') (OAG/train_paper_field.py:87) -- on the raw logits, forward and backward, one launch each.
//
//   hgt_class_loss      per row x of C logits: m = max x, ls = log(sum exp(x - m)), logp_j = (x_j - m) - ls, all fp32 as torch.log_softmax
//                       forms them; the row's term and its label weight W by one of three label forms:
//                         index y     term = -logp_y, W = 1;  y < 0: term 0, W 0 (ignored);  y >= C: NaN
//                         labels l    term = sum over l_j > 0 of l_j (log l_j - logp_j), W = sum l_j;  an entry < 0 or NaN: NaN
//                         columns     c = the number of entries >= 0 of the row's list: term = -log c - (1 / c) sum logp_col, W = 1
//                                     (c = 0: term 0, W 0);  an entry >= C, or count[r] > width: NaN
//                       (m, ls) is saved in its two parts, so that the backward forms (x - m) - ls exactly as the forward did.
//   hgt_class_loss_bwd  grad[r, j] = grad_loss[r] * (W_r * exp((x_j - m) - ls) - l_rj), every element of the C columns written once.
//
// A NaN term is saved with W = NaN, which makes the row's gradient NaN as well; a row with W = 0 (index < 0, an empty list) gets a
// gradient row of exact zeros whatever its logits hold.
//
// Rows of at most HGT_CLASS_LOSS_WAVE_COLS columns take a wavefront each: a lane holds four consecutive logits, the row is read once.
// Longer rows take a workgroup each and are streamed twice (max, then sum): the second pass of an 80 KB row comes from L2, and no row
// length is tied to the LDS size.  Position j of a row always belongs to the same thread -- 16-byte loads where the row's base is
// aligned, four scalar loads where it is not -- and the partial results are joined by a shuffle tree and then wavefront after
// wavefront, so a row's bits depend on the row alone: not on its alignment, n_rows, the other rows or the launch geometry.  The
// label-weighted terms are fp64, thread i taking entries i, i + T, ... of the row (dense: quads) before the same tree.  No atomics.
// Compiled without fast-math like the rest of the library.
#include <limits.h>
#include <math.h>

#include "hgt_common.h"
#include "hgt_row_common.h"

namespace {

struct ClassArgs {
    const float* x;
    const float* labels;
    const int64_t* index;
    const int32_t* columns;
    const int32_t* count;
    float* loss;                 // forward outputs
    float* lse;                  // [n_rows][2]: max, log(sum exp(x - max))
    float* wsum;
    const float* lse_in;         // backward inputs
    const float* wsum_in;
    const float* grad_loss;
    float* grad;
    int64_t ld, ld_l, ld_g;
    int32_t n_rows, n_cols, width;
};

struct Scratch {
    float f[CL_WAVES];
    double d[2][CL_WAVES];
    int i[2][CL_WAVES];
};

template <int T>
__device__ __forceinline__ int group_count(int v, Scratch& S) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if (T == 64) return v;
    if ((threadIdx.x & 63) == 0) S.i[0][threadIdx.x >> 6] = v;
    __syncthreads();
    v = S.i[0][0];
    for (int q = 1; q < CL_WAVES; ++q) v += S.i[0][q];
    __syncthreads();
    return v;
}

template <int T>
__device__ __forceinline__ void group_sum_terms(double& a, double& b, int& n, int& bad, Scratch& S) {
    for (int o = 32; o; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
        n += __shfl_xor(n, o);
        bad |= __shfl_xor(bad, o);
    }
    if (T == 64) return;
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        S.d[0][w] = a, S.d[1][w] = b, S.i[0][w] = n, S.i[1][w] = bad;
    }
    __syncthreads();
    a = S.d[0][0], b = S.d[1][0], n = S.i[0][0], bad = S.i[1][0];
    for (int q = 1; q < CL_WAVES; ++q) a += S.d[0][q], b += S.d[1][q], n += S.i[0][q], bad |= S.i[1][q];
    __syncthreads();
}

// T = 64: a wavefront per row of at most 256 columns, four rows a workgroup;  T = CL_BLOCK: a workgroup per row
template <int T>
__global__ void __launch_bounds__(CL_BLOCK) k_class_loss(ClassArgs A) {
    __shared__ Scratch S;
    const int k = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int r = T == 64 ? (int)(blockIdx.x * CL_WAVES + (threadIdx.x >> 6)) : (int)blockIdx.x;
    if (r >= A.n_rows) return;                                                    // uniform over the T threads, like every branch below
    const int C = A.n_cols;
    const float* x = A.x + (int64_t)r * A.ld;
    const bool vec = ((uintptr_t)x & 15) == 0;

    // ---- m and ls; a wavefront row stays in registers
    float own[4], m, ls;
    row_lse<T>(x, C, vec, k, own, S, m, ls);

    // ---- the label-weighted terms, fp64
    double acc = 0.0, w = 0.0;
    int n = 0, bad = 0;
    if (A.index) {
        const int64_t y = A.index[r];
        if (y >= C) {
            bad = 1;
        } else if (y >= 0) {
            if (k == 0) acc = -(double)((x[y] - m) - ls);
            w = k == 0 ? 1.0 : 0.0;
        }
    } else if (A.labels) {
        const float* l = A.labels + (int64_t)r * A.ld_l;
        const bool vec_l = ((uintptr_t)l & 15) == 0;
        for (int j = 4 * k; j < C; j += 4 * T) {
            float v[4];
            load4(l, j, C, vec_l, 0.0f, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (v[e] > 0.0f) {
                    const float logp = (x[j + e] - m) - ls;
                    acc += (double)v[e] * (log((double)v[e]) - (double)logp);
                    w += (double)v[e];
                } else if (!(v[e] >= 0.0f)) {                                     // negative or NaN
                    bad = 1;
                }
            }
        }
    } else {
        const int32_t* cols = A.columns + (int64_t)r * A.width;
        for (int i = k; i < A.width; i += T) {
            const int c = cols[i];
            if (c < 0) continue;
            ++n;
            if (c >= C) bad = 1;
            else acc += (double)((x[c] - m) - ls);
        }
        if (A.count && A.count[r] > A.width) bad = 1;
    }
    group_sum_terms<T>(acc, w, n, bad, S);
    if (k != 0) return;
    if (A.columns) {
        w = n ? 1.0 : 0.0;
        acc = n ? -log((double)n) - acc / (double)n : 0.0;
    }
    A.loss[r] = bad ? NAN : (float)acc;
    A.wsum[r] = bad ? NAN : (float)w;
    A.lse[2 * (int64_t)r] = m, A.lse[2 * (int64_t)r + 1] = ls;
}

template <int T>
__global__ void __launch_bounds__(CL_BLOCK) k_class_loss_bwd(ClassArgs A) {
    __shared__ Scratch S;
    const int k = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int r = T == 64 ? (int)(blockIdx.x * CL_WAVES + (threadIdx.x >> 6)) : (int)blockIdx.x;
    if (r >= A.n_rows) return;
    const int C = A.n_cols;
    const float* x = A.x + (int64_t)r * A.ld;
    const float* l = A.labels ? A.labels + (int64_t)r * A.ld_l : nullptr;
    float* out = A.grad + (int64_t)r * A.ld_g;
    const bool vec = ((uintptr_t)x & 15) == 0, vec_l = l && ((uintptr_t)l & 15) == 0, vec_o = ((uintptr_t)out & 15) == 0;
    const float m = A.lse_in[2 * (int64_t)r], ls = A.lse_in[2 * (int64_t)r + 1], W = A.wsum_in[r], g = A.grad_loss[r];
    const bool zero = !l && W == 0.0f;                                            // an ignored row: exact zeros
    const int64_t y = A.index ? A.index[r] : -1;

    // every column once; the columns of a list are written again below
    for (int j = 4 * k; j < C; j += 4 * T) {
        float v[4], lab[4], o[4];
        load4(x, j, C, vec, 0.0f, v);
        if (l) {
            load4(l, j, C, vec_l, 0.0f, lab);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) lab[e] = j + e == y ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = zero ? 0.0f : g * (W * expf((v[e] - m) - ls) - lab[e]);
        if (vec_o && j + 3 < C) {
            *reinterpret_cast<float4*>(out + j) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (j + e < C) out[j + e] = o[e];
            }
        }
    }
    if (!A.columns || zero) return;

    // the listed columns (distinct by contract): l = 1 / c there.  The stores above are complete before one of them is written again.
    const int32_t* cols = A.columns + (int64_t)r * A.width;
    int n = 0;
    for (int i = k; i < A.width; i += T) n += cols[i] >= 0;
    n = group_count<T>(n, S);
    __threadfence();
    if (T != 64) __syncthreads();
    const float lc = 1.0f / (float)n;
    for (int i = k; i < A.width; i += T) {
        const int c = cols[i];
        if (c >= 0 && c < C) out[c] = g * (W * expf((x[c] - m) - ls) - lc);
    }
}

int class_args_ok(const float* logits, int64_t ld, int32_t n_rows, int32_t n_cols, const float* labels, int64_t ld_labels,
                  const int64_t* index, const int32_t* columns, int32_t width, const int32_t* count) {
    if (n_rows < 0 || n_cols < 0 || width < 0) return HGT_ERR_INVALID_ARG;
    if ((labels != nullptr) + (index != nullptr) + (columns != nullptr) != 1) return HGT_ERR_INVALID_ARG;
    if (count && !columns) return HGT_ERR_INVALID_ARG;
    if (columns && width < 1) return HGT_ERR_INVALID_ARG;
    if (n_rows == 0) return HGT_OK;
    if (n_cols > INT_MAX - 4 * CL_BLOCK) return HGT_ERR_UNSUPPORTED;               // positions are 32-bit, a step past the end included
    if (n_cols > 0 && !logits) return HGT_ERR_INVALID_ARG;
    if (ld < n_cols || (labels && ld_labels < n_cols)) return HGT_ERR_INVALID_ARG;
    return HGT_OK;
}

}  // namespace

extern "C" int hgt_class_loss(const float* logits, int64_t ld, int32_t n_rows, int32_t n_cols, const float* labels, int64_t ld_labels,
                              const int64_t* index, const int32_t* columns, int32_t width, const int32_t* count, float* loss_out,
                              float* lse_out, float* wsum_out, void* stream) {
    const int rc = class_args_ok(logits, ld, n_rows, n_cols, labels, ld_labels, index, columns, width, count);
    if (rc != HGT_OK || n_rows == 0) return rc;
    if (!loss_out || !lse_out || !wsum_out) return HGT_ERR_INVALID_ARG;
    ClassArgs A = {};
    A.x = logits; A.labels = labels; A.index = index; A.columns = columns; A.count = count;
    A.loss = loss_out; A.lse = lse_out; A.wsum = wsum_out;
    A.ld = ld; A.ld_l = ld_labels; A.n_rows = n_rows; A.n_cols = n_cols; A.width = width;
    if (n_cols <= HGT_CLASS_LOSS_WAVE_COLS)
        k_class_loss<64><<<(unsigned)((n_rows + CL_WAVES - 1) / CL_WAVES), CL_BLOCK, 0, (hipStream_t)stream>>>(A);
    else
        k_class_loss<CL_BLOCK><<<(unsigned)n_rows, CL_BLOCK, 0, (hipStream_t)stream>>>(A);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_class_loss_bwd(const float* logits, int64_t ld, int32_t n_rows, int32_t n_cols, const float* labels, int64_t ld_labels,
                                  const int64_t* index, const int32_t* columns, int32_t width, const int32_t* count, const float* lse,
                                  const float* wsum, const float* grad_loss, float* grad_logits, int64_t ld_grad, void* stream) {
    const int rc = class_args_ok(logits, ld, n_rows, n_cols, labels, ld_labels, index, columns, width, count);
    if (rc != HGT_OK || n_rows == 0) return rc;
    if (!lse || !wsum || !grad_loss || (n_cols > 0 && !grad_logits) || ld_grad < n_cols) return HGT_ERR_INVALID_ARG;
    ClassArgs A = {};
    A.x = logits; A.labels = labels; A.index = index; A.columns = columns; A.count = count;
    A.lse_in = lse; A.wsum_in = wsum; A.grad_loss = grad_loss; A.grad = grad_logits;
    A.ld = ld; A.ld_l = ld_labels; A.ld_g = ld_grad; A.n_rows = n_rows; A.n_cols = n_cols; A.width = width;
    if (n_cols <= HGT_CLASS_LOSS_WAVE_COLS)
        k_class_loss_bwd<64><<<(unsigned)((n_rows + CL_WAVES - 1) / CL_WAVES), CL_BLOCK, 0, (hipStream_t)stream>>>(A);
    else
        k_class_loss_bwd<CL_BLOCK><<<(unsigned)n_rows, CL_BLOCK, 0, (hipStream_t)stream>>>(A);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}
