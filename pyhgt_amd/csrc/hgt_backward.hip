// Backward pass of HGTConv: the kernels that have no forward counterpart.  The reference gets its
// gradients from autograd through conv.py:60-134 (OAG/train_paper_field.py:249 `loss.backward()`); here the chain rule is
// written out on the node-level algebra of the forward so that the E x d tensors never exist either:
//
//   out = LN_t(y), y = o a + x (1 - a), a = sigmoid(skip_t), o = D * (gelu(agg) W_a^T + b_a)   (D = dropout mask / keep prob.)
//       -> hgt_node_update_bwd: d o, d x (skip path), d skip, d LN weight / bias
//       -> d gelu(agg) = d o W_a (typed linear with W_a^T), d agg = . * gelu'(agg) (hgt_gelu_bwd),
//          d W_a / d b_a = typed weight gradient (hgt_typed_wgrad / hgt_typed_colsum)
//   agg_i,h = sum_e att_e (v_e M_r):   d att_e = <dagg_i M_r^T, v_e>      = the LOGITS kernel with (Q, K, A') := (dagg, V, M^T)
//                                      d s_e   = att_e (d att_e - <dagg_i, agg_i>_h)                 (hgt_edge_softmax_bwd)
//   s_e = <A'_r q_i, k_e>:             d Q_i = sum_r (sum_e ds_e k_e) A'_r          = hgt_edge_spmm on the graph
//                                      d K_j = sum_r A'_r (sum_e ds_e q_i)          = hgt_edge_spmm on the TRANSPOSED graph
//                                      d V_j = sum_r (sum_e att_e dagg_i) M_r^T     = hgt_edge_spmm on the TRANSPOSED graph
//                                      d M_r = sum_e att_e v_e^T dagg_i,  d A'_r = sum_e ds_e k_e^T q_i   (hgt_relation_outer)
//   Q|K|V = x W_qkv^T + b:             d x += [dQ|dK|dV] W_qkv (typed linear), d W_qkv / d b_qkv = typed weight gradient.
// Everything is enqueued on the caller's stream; small parameter gradients are accumulated with fp32 atomics into
// caller-zeroed buffers (run-to-run differences of the summation order only).
//
// Deterministic forms (hgt_*_det, kernels k_det_*): the same kernel bodies instantiated with DET = true write each slot's partial
// result with plain stores into a workspace -- slot = a (group, row chunk) / a wavefront's row range / a slice of the plan's item
// list, all fixed on the host from the problem sizes (det_* functions below) -- and k_det_reduce sums the slots in slot order.
// No atomics, no waiting between workgroups: two launches on the stream are the ordering.
#include "hgt_edge_common.h"
#include "hgt_split_common.h"

namespace {


__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------------------------------------
// node update backward (conv.py:125-133 in reverse).  One wavefront per chunk of ROWS_PER_WAVE consecutive rows; the
// per-type parameter gradients are summed in registers while the type does not change and flushed with atomics.
// ---------------------------------------------------------------------------------------------
constexpr int NUB_ROWS = 32;
constexpr int NUB_MAXC = 8;          // columns per lane of k_node_update_bwd: d <= 512
constexpr int NUB_MAXC_WIDE = 16;    // ... of k_node_update_bwd_wide: 512 < d <= 1024 (like MAX_PER_LANE of the forward, hgt_update.hip)

template <int NUB_MAXC, bool DET = false>
__device__ __forceinline__ void node_update_bwd_rows(
    const float* __restrict__ gout, const float* __restrict__ trans, const float* __restrict__ x, int64_t ldx,
    const int64_t* __restrict__ node_type, const float* __restrict__ skip, const float* __restrict__ lnw, int use_norm,
    const float* __restrict__ drop_mask, int64_t NQ, int d, int T, float* __restrict__ d_trans, float* __restrict__ dx, int64_t ld_dx,
    float* __restrict__ d_alpha, float* __restrict__ d_lnw, float* __restrict__ d_lnb, int shared_norm, int rows_per_wave,
    int64_t det_slot_stride = 0) {
    // DET: d_lnw / d_lnb / d_alpha point into slot 0 of a zeroed workspace; this wavefront owns slot `wave` (plain read-modify-write)
    // skip == NULL: plain residual y = o + x (DenseHGTConv.update, conv.py:259,271), no gate gradient;
    // shared_norm: ONE LayerNorm for every type (out_norm, conv.py:272): its parameters / gradients are row 0 of lnw / d_lnw / d_lnb
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t r0 = wave * rows_per_wave;
    if (r0 >= NQ) return;
    if constexpr (DET) {
        if (d_lnw) d_lnw += wave * det_slot_stride;
        if (d_lnb) d_lnb += wave * det_slot_stride;
        if (d_alpha) d_alpha += wave * det_slot_stride;
    }
    const int nc = (d + 63) / 64;
    float gw[NUB_MAXC], gb[NUB_MAXC], ga = 0.0f;
#pragma unroll
    for (int c = 0; c < NUB_MAXC; ++c) gw[c] = gb[c] = 0.0f;
    int cur_t = -1;
    auto flush = [&]() {
        if (cur_t >= 0) {
            if (use_norm) {
#pragma unroll
                for (int c = 0; c < NUB_MAXC; ++c) {
                    const int col = c * 64 + lane;
                    if (c < nc && col < d) {
                        const int64_t lrow = shared_norm ? 0 : cur_t;
                        if constexpr (DET) {
                            d_lnw[lrow * d + col] += gw[c];
                            d_lnb[lrow * d + col] += gb[c];
                        } else {
                            unsafeAtomicAdd(&d_lnw[lrow * d + col], gw[c]);
                            unsafeAtomicAdd(&d_lnb[lrow * d + col], gb[c]);
                        }
                    }
                    gw[c] = gb[c] = 0.0f;
                }
            }
            if (skip) {
                ga = wave_sum(ga);
                if constexpr (DET) {
                    if (lane == 0) d_alpha[cur_t] += ga;
                } else {
                    if (lane == 0) unsafeAtomicAdd(&d_alpha[cur_t], ga);
                }
            }
            ga = 0.0f;
        }
    };
    for (int64_t r = r0; r < min(r0 + (int64_t)rows_per_wave, NQ); ++r) {
        const int64_t t64 = node_type[r];
        const int t = (t64 >= 0 && t64 < T) ? (int)t64 : -1;
        if (t != cur_t) { flush(); cur_t = t; }
        if (t < 0) {     // rows of unknown type: output 0, no gradient (conv.py:120)
#pragma unroll
            for (int c = 0; c < NUB_MAXC; ++c) {
                const int col = c * 64 + lane;
                if (c < nc && col < d) { d_trans[r * d + col] = 0.0f; dx[r * ld_dx + col] = 0.0f; }
            }
            continue;
        }
        const float alpha = skip ? 1.0f / (1.0f + expf(-skip[t])) : 1.0f;
        const float beta = skip ? 1.0f - alpha : 1.0f;           // weight of the residual row
        float o[NUB_MAXC], xv[NUB_MAXC], g[NUB_MAXC], y[NUB_MAXC];
        float s1 = 0.0f;
#pragma unroll
        for (int c = 0; c < NUB_MAXC; ++c) {
            const int col = c * 64 + lane;
            const bool ok = c < nc && col < d;
            o[c] = ok ? trans[r * d + col] : 0.0f;
            xv[c] = ok ? x[r * ldx + col] : 0.0f;
            g[c] = ok ? gout[r * d + col] : 0.0f;
            y[c] = o[c] * alpha + xv[c] * beta;
            s1 += y[c];
        }
        float dy[NUB_MAXC];
        if (use_norm) {
            const float mean = wave_sum(s1) / (float)d;
            float s2 = 0.0f;
#pragma unroll
            for (int c = 0; c < NUB_MAXC; ++c) {
                const int col = c * 64 + lane;
                const bool ok = c < nc && col < d;
                y[c] = ok ? y[c] - mean : 0.0f;
                s2 += y[c] * y[c];
            }
            const float rstd = rsqrtf(wave_sum(s2) / (float)d + 1e-5f);
            float a1 = 0.0f, a2 = 0.0f;
            float gh[NUB_MAXC];
#pragma unroll
            for (int c = 0; c < NUB_MAXC; ++c) {
                const int col = c * 64 + lane;
                const bool ok = c < nc && col < d;
                y[c] *= rstd;                                            // y = normalised row
                const float w = ok ? lnw[(int64_t)(shared_norm ? 0 : t) * d + col] : 0.0f;
                gw[c] += g[c] * y[c];
                gb[c] += g[c];
                gh[c] = g[c] * w;
                a1 += gh[c];
                a2 += gh[c] * y[c];
            }
            a1 = wave_sum(a1) / (float)d;
            a2 = wave_sum(a2) / (float)d;
#pragma unroll
            for (int c = 0; c < NUB_MAXC; ++c) dy[c] = rstd * (gh[c] - a1 - y[c] * a2);
        } else {
#pragma unroll
            for (int c = 0; c < NUB_MAXC; ++c) dy[c] = g[c];
        }
#pragma unroll
        for (int c = 0; c < NUB_MAXC; ++c) {
            const int col = c * 64 + lane;
            if (c < nc && col < d) {
                ga += dy[c] * (o[c] - xv[c]);
                float dt = dy[c] * alpha;
                if (drop_mask) dt *= drop_mask[r * d + col];            // o = mask * (a_linear output), conv.py:125
                d_trans[r * d + col] = dt;
                dx[r * ld_dx + col] = dy[c] * beta;
            }
        }
    }
    flush();
}

#define HGT_NUB_PARAMS                                                                                                              \
    const float *__restrict__ gout, const float *__restrict__ trans, const float *__restrict__ x, int64_t ldx,                       \
        const int64_t *__restrict__ node_type, const float *__restrict__ skip, const float *__restrict__ lnw, int use_norm,           \
        const float *__restrict__ drop_mask, int64_t NQ, int d, int T, float *__restrict__ d_trans, float *__restrict__ dx,            \
        int64_t ld_dx, float *__restrict__ d_alpha, float *__restrict__ d_lnw, float *__restrict__ d_lnb, int shared_norm,             \
        int rows_per_wave
#define HGT_NUB_ARGS \
    gout, trans, x, ldx, node_type, skip, lnw, use_norm, drop_mask, NQ, d, T, d_trans, dx, ld_dx, d_alpha, d_lnw, d_lnb, shared_norm, rows_per_wave

__global__ __launch_bounds__(256) void k_node_update_bwd(HGT_NUB_PARAMS) { node_update_bwd_rows<NUB_MAXC>(HGT_NUB_ARGS); }
// rows of 513 .. 1024 columns (n_hid 768 / 1024): the same walk with 16 columns per lane
__global__ __launch_bounds__(256) void k_node_update_bwd_wide(HGT_NUB_PARAMS) { node_update_bwd_rows<NUB_MAXC_WIDE>(HGT_NUB_ARGS); }
// deterministic forms: one workspace slot per wavefront (hgt_node_update_bwd_det)
__global__ __launch_bounds__(256) void k_det_node_update_bwd(HGT_NUB_PARAMS, int64_t det_slot_stride) {
    node_update_bwd_rows<NUB_MAXC, true>(HGT_NUB_ARGS, det_slot_stride);
}
__global__ __launch_bounds__(256) void k_det_node_update_bwd_wide(HGT_NUB_PARAMS, int64_t det_slot_stride) {
    node_update_bwd_rows<NUB_MAXC_WIDE, true>(HGT_NUB_ARGS, det_slot_stride);
}
#undef HGT_NUB_PARAMS
#undef HGT_NUB_ARGS

// Stage two of every deterministic form: out[seg][(i / per) * ogs + i % per] = sum of in[s][i] over the slots s of segment `seg`
// (blockIdx.y; seg_len slots each), in slot order.  One segment = the whole sum; many slots are summed in two passes (segments of
// DET_SEG slots into a scratch array, then the segments): still one fixed order, with enough threads to stream the partials.
constexpr int DET_SEG = 64, DET_TWO_PASS = 128;
__global__ __launch_bounds__(256) void k_det_reduce(const float* __restrict__ in, int n_slots, int64_t slot_stride, int64_t n_elems,
                                                    int seg_len, float* __restrict__ out, int64_t out_seg_stride, int64_t per,
                                                    int64_t ogs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_elems) return;
    const int s0 = blockIdx.y * seg_len, s1 = min(s0 + seg_len, n_slots);
    const float* p = in + (int64_t)s0 * slot_stride + i;
    float acc = 0.0f;
#pragma unroll 8
    for (int s = s0; s < s1; ++s, p += slot_stride) acc += *p;
    out[(int64_t)blockIdx.y * out_seg_stride + (i / per) * ogs + i % per] = acc;
}

// dagg = dg * gelu'(agg), gelu = exact erf form (conv.py:119)
__global__ void k_gelu_bwd(const float* __restrict__ dg, const float* __restrict__ agg, float* __restrict__ out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float4 a = *reinterpret_cast<const float4*>(agg + i);
    const float4 g = *reinterpret_cast<const float4*>(dg + i);
    auto f = [](float v, float gg) {
        const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
        const float pdf = 0.39894228040143267794f * __expf(-0.5f * v * v);
        return gg * (cdf + v * pdf);
    };
    *reinterpret_cast<float4*>(out + i) = make_float4(f(a.x, g.x), f(a.y, g.y), f(a.z, g.z), f(a.w, g.w));
}

// x[i] *= m[i]  (dropout of the a_linear output, conv.py:125; the mask holds 0 or 1/(1-p))
__global__ void k_mul_inplace(float* __restrict__ x, const float* __restrict__ m, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= m[i];
}

// ds[p][h] = att[p][h] * (datt[p][h] - rho[dst[p]][h])   (softmax backward per target and head; sorted edge order)
__global__ void k_edge_softmax_bwd(const int32_t* __restrict__ edst, const float* __restrict__ att, const float* __restrict__ datt,
                                   const float* __restrict__ rho, int64_t ld_rho, float* __restrict__ ds, int64_t E, int H) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E * H) return;
    const int64_t p = i / H;
    const int h = (int)(i % H);
    ds[i] = att[i] * (datt[i] - rho[(int64_t)edst[p] * ld_rho + h]);
}

// out[p][h] = in[eid[p]][h]: values in ORIGINAL edge order -> the sorted order of a plan
__global__ void k_gather_sorted(const int32_t* __restrict__ eid, const float* __restrict__ in, float* __restrict__ out, int64_t E, int H) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E * H) return;
    const int64_t p = i / H;
    out[i] = in[(int64_t)eid[p] * H + (i % H)];
}

// rho[n][h] = <a[n][h*dkp .. +dkp], b[n][...]>: a thread per 4 consecutive columns (coalesced 16 B loads of both rows), partial
// dots reduced over the dkp/4 consecutive threads of a head (dkp is a power of two)
__global__ void k_head_dot(const float* __restrict__ a, const float* __restrict__ b, int64_t n_rows, int H, int dkp, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // float4 index
    const int64_t total = n_rows * H * (dkp / 4);
    float s = 0.0f;
    if (i < total) {
        const float4 u = *reinterpret_cast<const float4*>(a + 4 * i);
        const float4 v = *reinterpret_cast<const float4*>(b + 4 * i);
        s = u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
    }
    const int tph = dkp / 4;                                               // threads per head: 1 .. 64
    for (int o = 1; o < tph; o <<= 1) s += __shfl_xor(s, o);
    if (i < total && (i % tph) == 0) out[i / tph] = s;
}

// ---------------------------------------------------------------------------------------------
// Typed weight gradient  dW[g][m][n] += sum_{rows p of group g} A[rows[p]][m] * B[rows[p]][n]   (= A_g^T B_g)
// on v_mfma_f32_32x32x2_f32 (exact fp32 products).  A workgroup owns a 64 x 64 tile of (m, n) and a chunk of WG_ROWS rows of
// one group: the 64-row slices of A and B go through LDS ([row][64] fp32), each wavefront owns a 32 x 32 quadrant, the
// partial tile is added to dW with fp32 atomics (one pass over every row per (m, n) tile: A is re-read n_out/64 times, B
// m/64 times -- fine for a one-off per step; the forward GEMMs are the optimised ones).
// ---------------------------------------------------------------------------------------------
constexpr int WG_ROWS = 2048;

// DET: chunk `slot % det_chunks` of the det_chunks equal row chunks (a multiple of `quantum` rows) of group `slot / det_chunks`
__device__ __forceinline__ void det_chunk_of(int slot, int det_chunks, int quantum, const int32_t* __restrict__ group_off, int& g,
                                             int& ch, int& p0, int& p1) {
    g = slot / det_chunks;
    ch = slot - g * det_chunks;
    const int gbeg = group_off[g], gend = group_off[g + 1];
    const int per = ((gend - gbeg + det_chunks - 1) / det_chunks + quantum - 1) / quantum * quantum;
    p0 = min(gbeg + ch * per, gend);
    p1 = min(p0 + per, gend);
}

template <bool DET>
__device__ __forceinline__ void typed_wgrad_body(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                 const int32_t* __restrict__ rows, const int32_t* __restrict__ group_off, int n_groups,
                                                 int M, int Nc, float* __restrict__ out, int64_t out_group_stride, int vecA, int vecB,
                                                 int det_chunks) {
    __shared__ float sA[64][68];
    __shared__ float sB[64][68];
    // which (group, row chunk) is this block?
    int slot = blockIdx.x, g = 0, gbeg = 0, gend = 0, before = 0;
    int p0, p1, det_ch = 0;
    if constexpr (DET) {
        det_chunk_of(slot, det_chunks, 64, group_off, g, det_ch, p0, p1);
    } else {
        for (; g < n_groups; ++g) {
            gbeg = group_off[g];
            gend = group_off[g + 1];
            const int nch = (gend - gbeg + WG_ROWS - 1) / WG_ROWS;
            if (slot < before + nch) break;
            before += nch;
        }
        if (g >= n_groups) return;
        p0 = gbeg + (slot - before) * WG_ROWS;
        p1 = min(p0 + WG_ROWS, gend);
    }
    const int m0 = blockIdx.y * 64, n0 = blockIdx.z * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int pb = p0; pb < p1; pb += 64) {
        __syncthreads();
        // 64 rows x 64 columns of A and of B: thread -> (row = tid / 4 .. , 16 columns)
        {
            const int r = tid >> 2, cq = (tid & 3) * 16;
            const int p = pb + r;
            const int64_t rid = (p < p1) ? (int64_t)rows[p] : -1;
#pragma unroll
            for (int j = 0; j < 16; j += 4) {
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                if (rid >= 0) {
                    const int ma = m0 + cq + j, nb = n0 + cq + j;
                    if (vecA && ma + 3 < M) a = *reinterpret_cast<const float4*>(A + rid * lda + ma);
                    else { if (ma < M) a.x = A[rid * lda + ma]; if (ma + 1 < M) a.y = A[rid * lda + ma + 1]; if (ma + 2 < M) a.z = A[rid * lda + ma + 2]; if (ma + 3 < M) a.w = A[rid * lda + ma + 3]; }
                    if (vecB && nb + 3 < Nc) b = *reinterpret_cast<const float4*>(B + rid * ldb + nb);
                    else { if (nb < Nc) b.x = B[rid * ldb + nb]; if (nb + 1 < Nc) b.y = B[rid * ldb + nb + 1]; if (nb + 2 < Nc) b.z = B[rid * ldb + nb + 2]; if (nb + 3 < Nc) b.w = B[rid * ldb + nb + 3]; }
                }
                *reinterpret_cast<float4*>(&sA[r][cq + j]) = a;
                *reinterpret_cast<float4*>(&sB[r][cq + j]) = b;
            }
        }
        __syncthreads();
        // D[m][n] += sum_row A[row][m] B[row][n]: MFMA operand a = A^T[m = lane&31][k = row], b = B[k = row][n = lane&31]
#pragma unroll 8
        for (int k = 0; k < 64; k += 2) {
            const int kr = k + (lane >> 5);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[kr][wm + (lane & 31)], sB[kr][wn + (lane & 31)], acc, 0, 0, 0);
        }
    }
    // C layout: col (n) = lane & 31, row (m) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    // DET: this chunk's own [n_groups][M][Nc] slot (out = the workspace, out_group_stride = M * Nc; one chunk: out itself)
    float* o = out + (int64_t)g * out_group_stride + (DET ? (int64_t)det_ch * n_groups * out_group_stride : 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), n = n0 + wn + (lane & 31);
        if (m < M && n < Nc) {
            if constexpr (DET) o[(int64_t)m * Nc + n] = acc[r];
            else unsafeAtomicAdd(&o[(int64_t)m * Nc + n], acc[r]);
        }
    }
}

__global__ __launch_bounds__(256) void k_typed_wgrad(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                     const int32_t* __restrict__ rows, const int32_t* __restrict__ group_off, int n_groups,
                                                     int M, int Nc, float* __restrict__ out, int64_t out_group_stride, int vecA, int vecB) {
    typed_wgrad_body<false>(A, lda, B, ldb, rows, group_off, n_groups, M, Nc, out, out_group_stride, vecA, vecB, 0);
}
__global__ __launch_bounds__(256) void k_det_typed_wgrad(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                         int64_t ldb, const int32_t* __restrict__ rows,
                                                         const int32_t* __restrict__ group_off, int n_groups, int M, int Nc,
                                                         float* __restrict__ out, int64_t out_group_stride, int vecA, int vecB,
                                                         int det_chunks) {
    typed_wgrad_body<true>(A, lda, B, ldb, rows, group_off, n_groups, M, Nc, out, out_group_stride, vecA, vecB, det_chunks);
}

// ---------------------------------------------------------------------------------------------
// The same weight gradient as 3-term split-bf16 products on v_mfma_f32_32x32x16_bf16 (relative error of a product ~3 * 2^-18, like
// the forward typed linears): 8x the matrix-core rate of the fp32 instruction and 128 x 128 output tiles, so that A and B are
// re-read Nc/128 and M/128 times instead of Nc/64 and M/64 (the fp32 kernel above moved 33 GB per training step at c2 = 11 ms).
// Both MFMA operands need the ROW index along K, i.e. eight consecutive rows of one column per lane: the 32-row chunks of A and B
// are therefore staged through LDS TRANSPOSED -- a thread reads eight rows of one column (coalesced 256 B per wavefront and row),
// splits them into bf16 hi / mid and writes one 16 B fragment piece per plane; column stride 80 B: conflict-free writes and reads.
// The next chunk's rows are in flight (registers) while the current one is multiplied.  Optionally also the column sums of A
// (bias gradient), from the registers that pass through anyway.
// ---------------------------------------------------------------------------------------------
constexpr int WX_T = 128;            // tile edge (columns of A = rows of dW, columns of B)
constexpr int WX_KR = 32;            // rows per chunk
constexpr int WX_CS = 80;            // LDS bytes per column: 32 rows x 2 B + 16 B of padding
constexpr int WX_PLANE = WX_T * WX_CS;
constexpr int WX_ROWS = 4096;        // rows of one group per workgroup

template <bool DET>
__device__ __forceinline__ void typed_wgrad_x3_body(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                    const int32_t* __restrict__ rows, const int32_t* __restrict__ group_off,
                                                    int n_groups, int M, int Nc, int n_mt, float* __restrict__ out,
                                                    int64_t out_group_stride, float* __restrict__ colsum, int64_t cs_group_stride,
                                                    int det_chunks) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * WX_PLANE];   // A hi | A mid | B hi | B mid
    // tile index fastest: the workgroups that share a row chunk are neighbours in launch order (their rows meet in the L2)
    const int mt = blockIdx.x % n_mt, nt = blockIdx.x / n_mt;
    int slot = blockIdx.y, g = 0, gbeg = 0, gend = 0, before = 0;
    int p0, p1, det_ch = 0;
    if constexpr (DET) {
        det_chunk_of(slot, det_chunks, WX_KR, group_off, g, det_ch, p0, p1);
    } else {
        for (; g < n_groups; ++g) {
            gbeg = group_off[g];
            gend = group_off[g + 1];
            const int nch = (gend - gbeg + WX_ROWS - 1) / WX_ROWS;
            if (slot < before + nch) break;
            before += nch;
        }
        if (g >= n_groups) return;
        p0 = gbeg + (slot - before) * WX_ROWS;
        p1 = min(p0 + WX_ROWS, gend);
    }
    const int m0 = mt * WX_T, n0 = nt * WX_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    // staging role: column c of the tile, row octets o0 and o0 + 2 of the chunk, for A and for B
    const int c = tid & 127, o0 = tid >> 7;
    const bool a_ok = m0 + c < M, b_ok = n0 + c < Nc;
    const float* __restrict__ pa = A + (a_ok ? m0 + c : 0);
    const float* __restrict__ pb = B + (b_ok ? n0 + c : 0);
    float va[16], vb[16];
    int rid[16], rid_next[16];       // row ids of the chunk in flight / of the one after it (no id -> row dependency inside the loop)
    auto load_ids = [&](int pbase, int (&ids)[16]) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int p = pbase + 8 * (o0 + 2 * (j >> 3)) + (j & 7);
            ids[j] = (p < p1) ? rows[p] : -1;
        }
    };
    auto load_rows = [&]() {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t r = max(rid[j], 0);
            va[j] = pa[r * lda];
            vb[j] = pb[r * ldb];
        }
    };
    float csum = 0.0f;
    auto commit = [&]() {       // registers -> transposed bf16 hi / mid planes (rows beyond the chunk and columns beyond M / Nc: 0)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float fa[8], fb[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool live = rid[half * 8 + j] >= 0;
                fa[j] = (live && a_ok) ? va[half * 8 + j] : 0.0f;
                fb[j] = (live && b_ok) ? vb[half * 8 + j] : 0.0f;
                csum += fa[j];
            }
            uint4 ah, am, bh, bm;
            split2(fa[0], fa[1], ah.x, am.x); split2(fa[2], fa[3], ah.y, am.y); split2(fa[4], fa[5], ah.z, am.z); split2(fa[6], fa[7], ah.w, am.w);
            split2(fb[0], fb[1], bh.x, bm.x); split2(fb[2], fb[3], bh.y, bm.y); split2(fb[4], fb[5], bh.z, bm.z); split2(fb[6], fb[7], bh.w, bm.w);
            unsigned char* w = smem + c * WX_CS + (o0 + 2 * half) * 16;
            *reinterpret_cast<uint4*>(w) = ah;
            *reinterpret_cast<uint4*>(w + WX_PLANE) = am;
            *reinterpret_cast<uint4*>(w + 2 * WX_PLANE) = bh;
            *reinterpret_cast<uint4*>(w + 3 * WX_PLANE) = bm;
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    load_ids(p0, rid);
    load_rows();
    load_ids(p0 + WX_KR, rid_next);
    for (int pbase = p0; pbase < p1; pbase += WX_KR) {
        __syncthreads();                 // the previous chunk's fragments have been read
        commit();
        if (pbase + WX_KR < p1) {        // next chunk's rows (in flight during the products below), the ids of the one after it
#pragma unroll
            for (int j = 0; j < 16; ++j) rid[j] = rid_next[j];
            load_rows();
            load_ids(pbase + 2 * WX_KR, rid_next);
        }
        __syncthreads();
        const unsigned char* fa = smem + (wm + (lane & 31)) * WX_CS + (lane >> 5) * 16;
        const unsigned char* fb = smem + 2 * WX_PLANE + (wn + (lane & 31)) * WX_CS + (lane >> 5) * 16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 ah[2], am[2], bh[2], bm[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *reinterpret_cast<const bf16x8*>(fa + i * 32 * WX_CS + ks * 32);
                am[i] = *reinterpret_cast<const bf16x8*>(fa + WX_PLANE + i * 32 * WX_CS + ks * 32);
                bh[i] = *reinterpret_cast<const bf16x8*>(fb + i * 32 * WX_CS + ks * 32);
                bm[i] = *reinterpret_cast<const bf16x8*>(fb + WX_PLANE + i * 32 * WX_CS + ks * 32);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
    }
    // C layout of a 32 x 32 tile: col (n) = lane & 31, row (m) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    // DET: this chunk's own [n_groups][M][Nc] / [n_groups][M] slots (out / colsum = the workspace; one chunk: the outputs themselves)
    float* o = out + (int64_t)g * out_group_stride + (DET ? (int64_t)det_ch * n_groups * out_group_stride : 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), n = n0 + wn + 32 * j + (lane & 31);
                if (m < M && n < Nc) {
                    if constexpr (DET) o[(int64_t)m * Nc + n] = acc[i][j][r];
                    else unsafeAtomicAdd(&o[(int64_t)m * Nc + n], acc[i][j][r]);
                }
            }
    if constexpr (DET) {
        // a column's sum sits in two threads (row octets o0 and o0 + 2 of every chunk): combined through LDS in a fixed order
        if (colsum && nt == 0) {      // (workgroup-uniform)
            float* s_cs = reinterpret_cast<float*>(smem);
            __syncthreads();          // the last chunk's fragments have been read
            if (o0 == 1) s_cs[c] = csum;
            __syncthreads();
            if (o0 == 0 && a_ok) colsum[((int64_t)det_ch * n_groups + g) * cs_group_stride + m0 + c] = csum + s_cs[c];
        }
    } else {
        if (colsum && nt == 0 && a_ok) unsafeAtomicAdd(&colsum[(int64_t)g * cs_group_stride + m0 + c], csum);
    }
}

__global__ __launch_bounds__(256) void k_typed_wgrad_x3(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                        const int32_t* __restrict__ rows, const int32_t* __restrict__ group_off,
                                                        int n_groups, int M, int Nc, int n_mt, float* __restrict__ out,
                                                        int64_t out_group_stride, float* __restrict__ colsum, int64_t cs_group_stride) {
    typed_wgrad_x3_body<false>(A, lda, B, ldb, rows, group_off, n_groups, M, Nc, n_mt, out, out_group_stride, colsum, cs_group_stride, 0);
}
__global__ __launch_bounds__(256) void k_det_typed_wgrad_x3(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                            int64_t ldb, const int32_t* __restrict__ rows,
                                                            const int32_t* __restrict__ group_off, int n_groups, int M, int Nc, int n_mt,
                                                            float* __restrict__ out, int64_t out_group_stride,
                                                            float* __restrict__ colsum, int64_t cs_group_stride, int det_chunks) {
    typed_wgrad_x3_body<true>(A, lda, B, ldb, rows, group_off, n_groups, M, Nc, n_mt, out, out_group_stride, colsum, cs_group_stride,
                              det_chunks);
}

// out[g][c] += sum_{rows p of group g} A[rows[p]][c]    (bias gradients)
__global__ __launch_bounds__(256) void k_typed_colsum(const float* __restrict__ A, int64_t lda, const int32_t* __restrict__ rows,
                                                      const int32_t* __restrict__ group_off, int n_groups, int M, float* __restrict__ out,
                                                      int64_t out_group_stride) {
    constexpr int CH = 256;
    int slot = blockIdx.x * 4 + (threadIdx.x >> 6), g = 0, gbeg = 0, gend = 0, before = 0;
    for (; g < n_groups; ++g) {
        gbeg = group_off[g];
        gend = group_off[g + 1];
        const int nch = (gend - gbeg + CH - 1) / CH;
        if (slot < before + nch) break;
        before += nch;
    }
    if (g >= n_groups) return;
    const int lane = threadIdx.x & 63;
    const int p0 = gbeg + (slot - before) * CH, p1 = min(p0 + CH, gend);
    for (int c0 = 0; c0 < M; c0 += 64 * 4) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int p = p0; p < p1; ++p) {
            const int64_t rid = rows[p];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j * 64 + lane;
                if (c < M) s[j] += A[rid * lda + c];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j * 64 + lane;
            if (c < M) unsafeAtomicAdd(&out[(int64_t)g * out_group_stride + c], s[j]);
        }
    }
}

// deterministic form: wavefront = chunk `slot % det_chunks` of group `slot / det_chunks`, its sums stored into the chunk's own
// [n_groups][out_group_stride] slot of `out` (the workspace; one chunk: the output itself)
__global__ __launch_bounds__(256) void k_det_typed_colsum(const float* __restrict__ A, int64_t lda, const int32_t* __restrict__ rows,
                                                          const int32_t* __restrict__ group_off, int n_groups, int M,
                                                          float* __restrict__ out, int64_t out_group_stride, int det_chunks) {
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= n_groups * det_chunks) return;
    int g, ch, p0, p1;
    det_chunk_of(slot, det_chunks, 1, group_off, g, ch, p0, p1);
    const int lane = threadIdx.x & 63;
    float* o = out + ((int64_t)ch * n_groups + g) * out_group_stride;
    for (int c0 = 0; c0 < M; c0 += 64 * 4) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int p = p0; p < p1; ++p) {
            const int64_t rid = rows[p];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + j * 64 + lane;
                if (c < M) s[j] += A[rid * lda + c];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j * 64 + lane;
            if (c < M) o[c] = s[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Relation outer products:  out[r][h][k][c] += sum_{e of relation r} w_e,h * a[src_e][h][k] * b[dst_e][h][c]
// (d relation_msg with (w, a, b) = (att, V, dagg); d A' with (ds, K, Q)).  A wavefront takes the work items of ONE relation
// (blockIdx.z) inside its slice of the plan's item list (runs of <= 512 sorted edges of one (tile, relation)); lane = (head,
// VEC rows k of the head's block); the b row of the edge is broadcast inside the head's lanes through LDS; the dkp x dkp
// blocks accumulate in registers over ~64 items and are flushed once with atomics.
// ---------------------------------------------------------------------------------------------
// DET (k_det_relation_outer*): the wavefront's blocks are STORED into its own [R][HT][dkp][dkp] slot of `out` (= the workspace;
// slot = the wavefront's slice of the item list, slices without an item of the relation store zeros) instead of added to out.
#define HGT_OUTER_PARAMS                                                                                                             \
    const HgtItem *__restrict__ items, const HgtPlanHeader *__restrict__ hdr, const int32_t *__restrict__ esrc,                        \
        const int32_t *__restrict__ edst, const uint16_t *__restrict__ ertei, const float *__restrict__ w, const float *__restrict__ a, \
        const float *__restrict__ rte_a, const float *__restrict__ b, float *__restrict__ out, int R, int HT, int items_per_wave
#define HGT_OUTER_ARGS items, hdr, esrc, edst, ertei, w, a, rte_a, b, out, R, HT, items_per_wave

template <int VEC, int LPH, bool RTE, bool DET>
__device__ __forceinline__ void relation_outer_body(HGT_OUTER_PARAMS) {
    constexpr int DKP = VEC * LPH, DP = 64 * VEC, H = 64 / LPH;
    __shared__ __attribute__((aligned(16))) float s_b[4][DP + 4 * (64 / LPH)];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hg = blockIdx.y;
    const int rel_sel = blockIdx.z;            // this wavefront only takes the items of ONE relation: one flush per wavefront
    const int64_t ld = (int64_t)HT * DKP;
    const int co = hg * DP;
    const int h = lane / LPH, p = lane % LPH;
    float* bounce = s_b[wib];
    const int n_items = hdr->n_items;
    const int first = (blockIdx.x * 4 + wib) * items_per_wave;
    if (!DET && first >= n_items) return;
    if constexpr (DET) out += (int64_t)(blockIdx.x * 4 + wib) * R * HT * DKP * DKP;
    float acc[VEC][DKP];      // rows k = p*VEC + i of head h, all DKP columns
#pragma unroll
    for (int i = 0; i < VEC; ++i)
#pragma unroll
        for (int c = 0; c < DKP; ++c) acc[i][c] = 0.0f;
    bool any = false;
    for (int ib = first; ib < min(first + items_per_wave, n_items); ib += 64) {
        // 64 item headers at a time (lane i = item ib + i); the matching ones are walked one after the other
        const int my_i = min(ib + lane, n_items - 1);
        const HgtItem mine = items[my_i];
        const bool take = (ib + lane < min(first + items_per_wave, n_items)) && mine.rel == rel_sel;
        unsigned long long todo = __builtin_amdgcn_ballot_w64(take);
        while (todo) {
            const int li_ = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int beg = __builtin_amdgcn_readlane(mine.beg, li_), end = __builtin_amdgcn_readlane(mine.end, li_);
            any = true;
            for (int base = beg; base < end; base += 64) {
                const int nb = min(64, end - base);
                const int li = base + min(lane, nb - 1);
                const int my_src = esrc[li], my_dst = edst[li];
                const int my_rte = RTE ? (int)ertei[li] : 0;
                // UB edges per batch: all their row / weight loads are issued (unconditionally: slots beyond the chunk re-read
                // its last edge) before the first one is consumed -- one memory round trip per batch instead of one per edge
                // (the per-edge form ran 15.7 ms at c2, the whole backward pass 68 ms)
                constexpr int UB = (VEC * DKP <= 128 && !RTE) ? 8 : 4;      // (more would push the kernel past 256 registers = one wavefront per SIMD)
                for (int e0 = 0; e0 < nb; e0 += UB) {
                    float av[UB][VEC], bv[UB][VEC], tv[RTE ? UB : 1][VEC], we[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const int idx = min(e0 + u, nb - 1);
                        const int s = __builtin_amdgcn_readlane(my_src, idx), dd = __builtin_amdgcn_readlane(my_dst, idx);
                        load_vec<VEC>(a + (int64_t)s * ld + co + lane * VEC, av[u]);
                        if constexpr (RTE) {
                            const int ri = __builtin_amdgcn_readlane(my_rte, idx);
                            load_vec<VEC>(rte_a + (int64_t)ri * ld + co + lane * VEC, tv[u]);
                        }
                        load_vec<VEC>(b + (int64_t)dd * ld + co + lane * VEC, bv[u]);
                        we[u] = w[(int64_t)(base + idx) * HT + hg * H + h];
                    }
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        if (e0 + u < nb) {
#pragma unroll
                            for (int i = 0; i < VEC; ++i) {
                                if constexpr (RTE) av[u][i] += tv[u][i];
                                av[u][i] *= we[u];
                            }
                            store_vec_lds<VEC>(bounce + lane * VEC + (lane / LPH) * 4, bv[u]);
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                            const float* xb = bounce + h * (DKP + 4);
#pragma unroll
                            for (int c4 = 0; c4 < DKP / 4; ++c4) {
                                const float4 bb = *reinterpret_cast<const float4*>(xb + 4 * c4);
#pragma unroll
                                for (int i = 0; i < VEC; ++i) {
                                    acc[i][4 * c4 + 0] = fmaf(av[u][i], bb.x, acc[i][4 * c4 + 0]);
                                    acc[i][4 * c4 + 1] = fmaf(av[u][i], bb.y, acc[i][4 * c4 + 1]);
                                    acc[i][4 * c4 + 2] = fmaf(av[u][i], bb.z, acc[i][4 * c4 + 2]);
                                    acc[i][4 * c4 + 3] = fmaf(av[u][i], bb.w, acc[i][4 * c4 + 3]);
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                        }
                    }
                }
            }
        }
    }
    if (any || DET) {
        float* o = out + (((int64_t)rel_sel * HT + hg * H + h) * DKP + p * VEC) * DKP;
#pragma unroll
        for (int i = 0; i < VEC; ++i)
#pragma unroll
            for (int c = 0; c < DKP; ++c) {
                if constexpr (DET) o[i * DKP + c] = acc[i][c];
                else unsafeAtomicAdd(&o[i * DKP + c], acc[i][c]);
            }
    }
}
template <int VEC, int LPH, bool RTE>
__global__ __launch_bounds__(256) void k_relation_outer(HGT_OUTER_PARAMS) { relation_outer_body<VEC, LPH, RTE, false>(HGT_OUTER_ARGS); }
template <int VEC, int LPH, bool RTE>
__global__ __launch_bounds__(256) void k_det_relation_outer(HGT_OUTER_PARAMS) { relation_outer_body<VEC, LPH, RTE, true>(HGT_OUTER_ARGS); }

// The same sums on the matrix cores for 32-wide heads (d_k = 32: c2, c3): the outer products of an edge batch are one
// v_mfma_f32_32x32x2_f32 per (head, pair of edges) -- operand A = the two scaled source rows' 32 head columns, B = the two target
// rows' -- exact fp32 products, 256 matrix-core cycles per edge instead of ~550 vector-ALU cycles (128 FMAs per lane, LDS bounce,
// two wave barriers per edge).  The rows of a batch are parked in LDS as [edge][column] (288-float stride: the two edges of a pair
// fall into different bank halves); the 8 head blocks accumulate in 128 registers and are flushed once per wavefront.
template <int VEC, bool RTE, bool DET>
__device__ __forceinline__ void relation_outer_mfma_body(HGT_OUTER_PARAMS) {
    constexpr int DKP = 32, LPH = DKP / VEC, DP = 64 * VEC, H = 64 / LPH, UB = 8, RS = DP + 32;   // RS: LDS row stride in floats
    static_assert(DP % 32 == 0 && H * DKP == DP, "32-wide heads");
    __shared__ __attribute__((aligned(16))) float s_rows[4][2][UB][RS];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hg = blockIdx.y, rel_sel = blockIdx.z;
    const int64_t ld = (int64_t)HT * DKP;
    const int co = hg * DP;
    const int h = lane / LPH;
    float (*sa)[RS] = s_rows[wib][0];
    float (*sb)[RS] = s_rows[wib][1];
    const int n_items = hdr->n_items;
    const int first = (blockIdx.x * 4 + wib) * items_per_wave;
    if (!DET && first >= n_items) return;
    if constexpr (DET) out += (int64_t)(blockIdx.x * 4 + wib) * R * HT * DKP * DKP;
    f32x16 acc[H];
#pragma unroll
    for (int hh = 0; hh < H; ++hh)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[hh][r] = 0.0f;
    bool any = false;
    for (int ib = first; ib < min(first + items_per_wave, n_items); ib += 64) {
        const int my_i = min(ib + lane, n_items - 1);
        const HgtItem mine = items[my_i];
        const bool take = (ib + lane < min(first + items_per_wave, n_items)) && mine.rel == rel_sel;
        unsigned long long todo = __builtin_amdgcn_ballot_w64(take);
        while (todo) {
            const int li_ = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int beg = __builtin_amdgcn_readlane(mine.beg, li_), end = __builtin_amdgcn_readlane(mine.end, li_);
            any = true;
            for (int base = beg; base < end; base += 64) {
                const int nb = min(64, end - base);
                const int li = base + min(lane, nb - 1);
                const int my_src = esrc[li], my_dst = edst[li];
                const int my_rte = RTE ? (int)ertei[li] : 0;
                for (int e0 = 0; e0 < nb; e0 += UB) {
                    float av[UB][VEC], bv[UB][VEC], tv[RTE ? UB : 1][VEC], we[UB];
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const int idx = min(e0 + u, nb - 1);
                        const int s = __builtin_amdgcn_readlane(my_src, idx), dd = __builtin_amdgcn_readlane(my_dst, idx);
                        load_vec<VEC>(a + (int64_t)s * ld + co + lane * VEC, av[u]);
                        if constexpr (RTE) {
                            const int ri = __builtin_amdgcn_readlane(my_rte, idx);
                            load_vec<VEC>(rte_a + (int64_t)ri * ld + co + lane * VEC, tv[u]);
                        }
                        load_vec<VEC>(b + (int64_t)dd * ld + co + lane * VEC, bv[u]);
                        we[u] = w[(int64_t)(base + idx) * HT + hg * H + h];
                    }
                    __builtin_amdgcn_wave_barrier();          // the previous batch's operands have been read
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        const float sc = (e0 + u < nb) ? we[u] : 0.0f;      // slots beyond the chunk contribute nothing
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            if constexpr (RTE) av[u][i] += tv[u][i];
                            av[u][i] *= sc;
                        }
                        store_vec_lds<VEC>(&sa[u][lane * VEC], av[u]);
                        store_vec_lds<VEC>(&sb[u][lane * VEC], bv[u]);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const int er = lane >> 5, cc = lane & 31;
#pragma unroll
                    for (int hh = 0; hh < H; ++hh)
#pragma unroll
                        for (int pr = 0; pr < UB / 2; ++pr)
                            acc[hh] = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[2 * pr + er][hh * 32 + cc], sb[2 * pr + er][hh * 32 + cc], acc[hh],
                                                                          0, 0, 0);
                }
            }
        }
    }
    if (any || DET) {
        // C layout of a 32 x 32 block: column c = lane & 31, row k = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int hh = 0; hh < H; ++hh) {
            float* o = out + ((int64_t)rel_sel * HT + hg * H + hh) * DKP * DKP;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if constexpr (DET) o[k * DKP + (lane & 31)] = acc[hh][r];
                else unsafeAtomicAdd(&o[k * DKP + (lane & 31)], acc[hh][r]);
            }
        }
    }
}
template <int VEC, bool RTE>
__global__ __launch_bounds__(256, 2) void k_relation_outer_mfma(HGT_OUTER_PARAMS) { relation_outer_mfma_body<VEC, RTE, false>(HGT_OUTER_ARGS); }
template <int VEC, bool RTE>
__global__ __launch_bounds__(256, 2) void k_det_relation_outer_mfma(HGT_OUTER_PARAMS) { relation_outer_mfma_body<VEC, RTE, true>(HGT_OUTER_ARGS); }
#undef HGT_OUTER_PARAMS
#undef HGT_OUTER_ARGS

// items of the plan per wavefront of the atomic form (a function of the plan's sizes)
static inline int outer_items_per_wave(int64_t max_items, int R) { return (max_items < 16384 ? 2 : 16) * (R + 1); }

template <int VEC, int LPH>
struct LaunchOuter {
    // det_ipw > 0: the deterministic form with det_ipw items per wavefront, `out` = the workspace (one slot per wavefront)
    static int run(const HgtPlanView& pv, const float* w, const float* a, const float* rte_a, const float* b, float* out, int R, int HT,
                   hipStream_t stream, int det_ipw = 0) {
        if constexpr (VEC * LPH * VEC <= 128 && VEC * LPH >= 4) {
            if (det_ipw > 0) {
                const int64_t dwaves = (pv.L.max_items + det_ipw - 1) / det_ipw;
                dim3 dgrid((unsigned)((dwaves + 3) / 4), (unsigned)(HT / (64 / LPH)), (unsigned)R);
                if constexpr (VEC * LPH == 32 && VEC <= 4) {
                    if (rte_a)
                        k_det_relation_outer_mfma<VEC, true><<<dgrid, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, w, a,
                                                                                       rte_a, b, out, R, HT, det_ipw);
                    else
                        k_det_relation_outer_mfma<VEC, false><<<dgrid, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, w, a,
                                                                                        rte_a, b, out, R, HT, det_ipw);
                    return HGT_OK;
                }
                if (rte_a)
                    k_det_relation_outer<VEC, LPH, true><<<dgrid, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, w, a, rte_a,
                                                                                   b, out, R, HT, det_ipw);
                else
                    k_det_relation_outer<VEC, LPH, false><<<dgrid, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, w, a, rte_a,
                                                                                    b, out, R, HT, det_ipw);
                return HGT_OK;
            }
            // ~16 items of the selected relation per wavefront (items are ordered (tile, relation)): at c2 3 000 wavefronts for
            // 1 024 SIMDs (64 items left the chip with fewer wavefronts than SIMDs) against 25 M flush atomics
            // (sampled batches -- a few thousand 16-edge items: 16 (R + 1) items per wavefront left 13 x R wavefronts walking ~250 edges
            //  each, 565 us per call at c3 (r6 timeline of a training step); 2 (R + 1) there)
            const int ipw = outer_items_per_wave(pv.L.max_items, R);
            const int64_t waves = (pv.L.max_items + ipw - 1) / ipw;
            dim3 grid((unsigned)((waves + 3) / 4), (unsigned)(HT / (64 / LPH)), (unsigned)R);
            if constexpr (VEC * LPH == 32 && VEC <= 4) {          // 32-wide heads: matrix-core form
                if (rte_a)
                    k_relation_outer_mfma<VEC, true><<<grid, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, w, a, rte_a, b, out,
                                                                              R, HT, ipw);
                else
                    k_relation_outer_mfma<VEC, false><<<grid, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, w, a, rte_a, b, out,
                                                                               R, HT, ipw);
                return HGT_OK;
            }
            if (rte_a)
                k_relation_outer<VEC, LPH, true><<<grid, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, w, a, rte_a, b, out, R,
                                                                          HT, ipw);
            else
                k_relation_outer<VEC, LPH, false><<<grid, 256, 0, stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, w, a, rte_a, b, out, R,
                                                                           HT, ipw);
            return HGT_OK;
        } else {
            return HGT_ERR_UNSUPPORTED;
        }
    }
};

// Heads of 128 and 256 padded columns (hgt_relation_outer_wide): per head the sum is a dkp x dkp GEMM whose reduction dimension is
// the relation's edges -- far past what a wavefront's registers hold, so a WORKGROUP owns one 128 x 128 block of one head of one
// relation (blockIdx.y = (head, row block, column block), blockIdx.z = relation) and its four wavefronts the four 64 x 64 quadrants:
// 2 x 2 v_mfma_f32_32x32x2_f32 accumulators each (exact fp32 products, 64 registers).  The workgroup walks the matching items of
// its slice of the item list; per batch of OW_UB edges its 256 threads gather the 128-column segments of the source rows (+ temporal
// rows), scale them with the edge weight and park them next to the target rows' segments in LDS ([edge][column], stride 160 floats:
// the two edges of an MFMA pair fall into different bank halves), so a segment is read from memory once per block instead of once
// per quadrant.  Two LDS buffers: one barrier per batch; the next batch of the item is fetched while the matrix cores run.
constexpr int OW_UB = 16;             // edges per batch (two per thread and operand)
constexpr int OW_RS = 128 + 32;       // LDS row stride in floats
constexpr int OW_ITEMS_SMALL = 8, OW_ITEMS_LARGE = 64;   // items per workgroup = this x (R + 1): LaunchOuter's 2 / 16 per wavefront x 4

struct OwBatch {                      // one thread's share of a batch: 4 columns of two edges' rows, and the edges' weights
    float4 a[2], t[2], b[2];
    float w[2];
};

#define HGT_OUTER_WIDE_PARAMS                                                                                                        \
    const HgtItem *__restrict__ items, const HgtPlanHeader *__restrict__ hdr, const int32_t *__restrict__ esrc,                        \
        const int32_t *__restrict__ edst, const uint16_t *__restrict__ ertei, const float *__restrict__ w, const float *__restrict__ a, \
        const float *__restrict__ rte_a, const float *__restrict__ b, float *__restrict__ out, int HT, int dkp, int items_per_wg
// DET (k_det_relation_outer_wide): the workgroup's block is STORED into slot blockIdx.x ([gridDim.z][HT][dkp][dkp]) of `out` (= the
// workspace); a slice without an item of the relation stores zeros
template <bool RTE, bool DET>
__device__ __forceinline__ void relation_outer_wide_body(HGT_OUTER_WIDE_PARAMS) {
    __shared__ __attribute__((aligned(16))) float s_rows[2][2][OW_UB][OW_RS];      // [buffer][a | b][edge][column]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nblk_h = dkp / 128;                              // 128-column blocks per head side: 1 or 2
    const int h = blockIdx.y / (nblk_h * nblk_h);
    const int kb = (blockIdx.y / nblk_h) % nblk_h, cb = blockIdx.y % nblk_h;
    const int rel_sel = blockIdx.z;
    const int64_t ld = (int64_t)HT * dkp;
    const int n_items = hdr->n_items;
    const int first = blockIdx.x * items_per_wg;
    if (!DET && first >= n_items) return;
    if constexpr (DET) out += (int64_t)blockIdx.x * gridDim.z * HT * dkp * dkp;
    const int last = min(first + items_per_wg, n_items);
    // gather role: thread = (edge slot u of the batch (and u + 8), 4 columns)
    const int u = tid >> 5, c4 = (tid & 31) * 4;
    const float* a_seg = a + h * dkp + kb * 128 + c4;
    const float* t_seg = RTE ? rte_a + h * dkp + kb * 128 + c4 : nullptr;
    const float* b_seg = b + h * dkp + cb * 128 + c4;
    // matrix-core role: wavefront = quadrant (qr, qc); lane = (edge of the pair, row / column inside a 32-wide tile)
    const int qr = wib >> 1, qc = wib & 1;
    const int er = lane >> 5, cc = lane & 31;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    OwBatch bt;
    auto fetch = [=](int e0, int end) {
        OwBatch n;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = e0 + u + 8 * k;
            const int idx = min(e, end - 1);           // slots beyond the item re-read its last edge with weight 0
            const int s = esrc[idx], dd = edst[idx];
            n.a[k] = *reinterpret_cast<const float4*>(a_seg + (int64_t)s * ld);
            if constexpr (RTE) n.t[k] = *reinterpret_cast<const float4*>(t_seg + (int64_t)ertei[idx] * ld);
            else n.t[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // (never read: a fully written struct stays in registers)
            n.b[k] = *reinterpret_cast<const float4*>(b_seg + (int64_t)dd * ld);
            n.w[k] = e < end ? w[(int64_t)idx * HT + h] : 0.0f;
        }
        return n;
    };
    int buf = 0;
    bool any = false;
    for (int ib = first; ib < last; ib += 64) {
        // 64 item headers at a time (lane i = item ib + i), the same in every wavefront: the loops below are workgroup-uniform
        const HgtItem mine = items[min(ib + lane, n_items - 1)];
        const bool take = (ib + lane < last) && mine.rel == rel_sel;
        unsigned long long todo = __builtin_amdgcn_ballot_w64(take);
        while (todo) {
            const int li_ = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int beg = __builtin_amdgcn_readlane(mine.beg, li_), end = __builtin_amdgcn_readlane(mine.end, li_);
            if (beg >= end) continue;
            any = true;
            bt = fetch(beg, end);
            for (int e0 = beg; e0 < end; e0 += OW_UB) {
                float (*sa)[OW_RS] = s_rows[buf][0];
                float (*sb)[OW_RS] = s_rows[buf][1];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    float4 v = bt.a[k];
                    if constexpr (RTE) { v.x += bt.t[k].x; v.y += bt.t[k].y; v.z += bt.t[k].z; v.w += bt.t[k].w; }
                    v.x *= bt.w[k]; v.y *= bt.w[k]; v.z *= bt.w[k]; v.w *= bt.w[k];
                    *reinterpret_cast<float4*>(&sa[u + 8 * k][c4]) = v;
                    *reinterpret_cast<float4*>(&sb[u + 8 * k][c4]) = bt.b[k];
                }
                // one barrier per batch: this buffer was last read two batches ago, before the previous batch's barrier
                __syncthreads();
                if (e0 + OW_UB < end) bt = fetch(e0 + OW_UB, end);
#pragma unroll
                for (int pr = 0; pr < OW_UB / 2; ++pr) {
                    float fa[2], fb[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        fa[i] = sa[2 * pr + er][qr * 64 + i * 32 + cc];
                        fb[i] = sb[2 * pr + er][qc * 64 + i * 32 + cc];
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
                }
                buf ^= 1;
            }
        }
    }
    if (any || DET) {
        // C layout of a 32 x 32 tile: column c = lane & 31, row k = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        float* o = out + (((int64_t)rel_sel * HT + h) * dkp + kb * 128 + qr * 64) * dkp + cb * 128 + qc * 64;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * er;
                    if constexpr (DET) o[(int64_t)k * dkp + j * 32 + cc] = acc[i][j][r];
                    else unsafeAtomicAdd(&o[(int64_t)k * dkp + j * 32 + cc], acc[i][j][r]);
                }
    }
}
template <bool RTE>
__global__ __launch_bounds__(256, 2) void k_relation_outer_wide(HGT_OUTER_WIDE_PARAMS) {
    relation_outer_wide_body<RTE, false>(items, hdr, esrc, edst, ertei, w, a, rte_a, b, out, HT, dkp, items_per_wg);
}
template <bool RTE>
__global__ __launch_bounds__(256, 2) void k_det_relation_outer_wide(HGT_OUTER_WIDE_PARAMS) {
    relation_outer_wide_body<RTE, true>(items, hdr, esrc, edst, ertei, w, a, rte_a, b, out, HT, dkp, items_per_wg);
}
#undef HGT_OUTER_WIDE_PARAMS

static inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

static int node_update_bwd_impl(const float* grad_out, const float* trans, const float* x, int64_t ldx, const int64_t* node_type,
                                const float* skip, const float* ln_w, int32_t use_norm, int32_t shared_norm, const float* drop_mask,
                                int64_t n_rows, int32_t d, int32_t n_types, float* d_trans, float* dx, int64_t ld_dx, float* d_alpha,
                                float* d_ln_w, float* d_ln_b, void* stream) {
    if (!grad_out || !trans || !x || !node_type || !d_trans || !dx || (skip && !d_alpha) || n_rows < 0 || d <= 0 || d > 64 * NUB_MAXC_WIDE)
        return HGT_ERR_INVALID_ARG;
    if (use_norm && (!ln_w || !d_ln_w || !d_ln_b)) return HGT_ERR_INVALID_ARG;
    if (n_rows == 0) return HGT_OK;
    // rows per wavefront: 32 amortise the parameter-gradient atomics on a large graph; a sampled batch of a few thousand rows would be
    // ~100 wavefronts walking 32 rows one after the other (c3: 119 us) -- 2 rows there, 8 in between
    const int rpw = n_rows >= 65536 ? NUB_ROWS : (n_rows >= 16384 ? 8 : 2);
    const int64_t waves = (n_rows + rpw - 1) / rpw;
    // d <= 512 keeps the 8-columns-per-lane kernel (its registers, its results); wider rows take the 16-column instantiation
    auto* kernel = d <= 64 * NUB_MAXC ? k_node_update_bwd : k_node_update_bwd_wide;
    kernel<<<nblk(waves, 4), 256, 0, (hipStream_t)stream>>>(grad_out, trans, x, ldx, node_type, skip, ln_w, use_norm, drop_mask, n_rows, d,
                                                            n_types, d_trans, dx, ld_dx, d_alpha, d_ln_w, d_ln_b, shared_norm, rpw);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_node_update_bwd(const float* grad_out, const float* trans, const float* x, int64_t ldx, const int64_t* node_type,
                                   const float* skip, const float* ln_w, int32_t use_norm, const float* drop_mask, int64_t n_rows,
                                   int32_t d, int32_t n_types, float* d_trans, float* dx, int64_t ld_dx, float* d_alpha, float* d_ln_w,
                                   float* d_ln_b, void* stream) {
    if (!skip) return HGT_ERR_INVALID_ARG;
    return node_update_bwd_impl(grad_out, trans, x, ldx, node_type, skip, ln_w, use_norm, 0, drop_mask, n_rows, d, n_types, d_trans, dx,
                                ld_dx, d_alpha, d_ln_w, d_ln_b, stream);
}

// reverse of hgt_node_update_ex: skip == NULL = plain residual (no gate, d_alpha unused), shared_norm = one LayerNorm for all types
extern "C" int hgt_node_update_bwd_ex(const float* grad_out, const float* trans, const float* x, int64_t ldx, const int64_t* node_type,
                                      const float* skip, const float* ln_w, int32_t use_norm, int32_t shared_norm, const float* drop_mask,
                                      int64_t n_rows, int32_t d, int32_t n_types, float* d_trans, float* dx, int64_t ld_dx,
                                      float* d_alpha, float* d_ln_w, float* d_ln_b, void* stream) {
    return node_update_bwd_impl(grad_out, trans, x, ldx, node_type, skip, ln_w, use_norm, shared_norm, drop_mask, n_rows, d, n_types,
                                d_trans, dx, ld_dx, d_alpha, d_ln_w, d_ln_b, stream);
}

// off2 = {0, off[n_groups]}: every row of a valid group as ONE group (the shared dense layer of DenseHGTConv)
__global__ void k_single_group_offsets(const int32_t* __restrict__ off, int n_groups, int32_t* __restrict__ off2) {
    if (threadIdx.x == 0) { off2[0] = 0; off2[1] = off[n_groups]; }
}
extern "C" int hgt_single_group_offsets(const int32_t* group_off, int32_t n_groups, int32_t* off2, void* stream) {
    if (!group_off || !off2 || n_groups <= 0) return HGT_ERR_INVALID_ARG;
    k_single_group_offsets<<<1, 64, 0, (hipStream_t)stream>>>(group_off, n_groups, off2);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_gelu_bwd(const float* dg, const float* agg, float* out, int64_t n, void* stream) {
    if (!dg || !agg || !out || n < 0 || (n & 3) != 0) return HGT_ERR_INVALID_ARG;
    if (n == 0) return HGT_OK;
    k_gelu_bwd<<<nblk(n / 4, 256), 256, 0, (hipStream_t)stream>>>(dg, agg, out, n);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_mul_inplace(float* x, const float* m, int64_t n, void* stream) {
    if (!x || !m || n < 0) return HGT_ERR_INVALID_ARG;
    if (n == 0) return HGT_OK;
    k_mul_inplace<<<nblk(n, 256), 256, 0, (hipStream_t)stream>>>(x, m, n);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_edge_softmax_bwd(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, const float* att,
                                    const float* d_att, const float* rho, int64_t ld_rho, float* d_logits, void* stream) {
    if (!plan || !att || !d_att || !rho || !d_logits || H <= 0) return HGT_ERR_INVALID_ARG;
    if (E == 0) return HGT_OK;
    HgtPlanView pv = hgt_plan_view(plan, N, E, T, R);
    k_edge_softmax_bwd<<<nblk(E * H, 256), 256, 0, (hipStream_t)stream>>>(pv.edst, att, d_att, rho, ld_rho, d_logits, E, H);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_edge_gather_sorted(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, const float* by_edge_id,
                                      float* sorted, void* stream) {
    if (!plan || !by_edge_id || !sorted || H <= 0) return HGT_ERR_INVALID_ARG;
    if (E == 0) return HGT_OK;
    HgtPlanView pv = hgt_plan_view(plan, N, E, T, R);
    k_gather_sorted<<<nblk(E * H, 256), 256, 0, (hipStream_t)stream>>>(pv.eid, by_edge_id, sorted, E, H);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_head_dot(const float* a, const float* b, int64_t n_rows, int32_t n_heads, int32_t dk_pad, float* out, void* stream) {
    if (!a || !b || !out || n_rows < 0 || n_heads <= 0 || dk_pad <= 0 || (dk_pad & 3) != 0) return HGT_ERR_INVALID_ARG;
    if (n_rows == 0) return HGT_OK;
    if (dk_pad > 256 || (dk_pad & (dk_pad - 1)) != 0) return HGT_ERR_INVALID_ARG;
    k_head_dot<<<nblk(n_rows * n_heads * (dk_pad / 4), 256), 256, 0, (hipStream_t)stream>>>(a, b, n_rows, n_heads, dk_pad, out);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_typed_wgrad(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows, const int32_t* group_off,
                               int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, float* out, int64_t out_group_stride,
                               void* stream) {
    if (!A || !B || !rows || !group_off || !out || n_groups <= 0 || n_rows < 0 || m <= 0 || n_cols <= 0) return HGT_ERR_INVALID_ARG;
    const int vecA = ((lda & 3) == 0 && ((uintptr_t)A & 15) == 0), vecB = ((ldb & 3) == 0 && ((uintptr_t)B & 15) == 0);   // 16 B row loads
    if (n_rows == 0) return HGT_OK;
    const int64_t chunks = (n_rows + WG_ROWS - 1) / WG_ROWS + n_groups;   // device-side group sizes: launch the upper bound
    dim3 grid((unsigned)chunks, (unsigned)((m + 63) / 64), (unsigned)((n_cols + 63) / 64));
    k_typed_wgrad<<<grid, 256, 0, (hipStream_t)stream>>>(A, lda, B, ldb, rows, group_off, n_groups, m, n_cols, out, out_group_stride, vecA, vecB);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_typed_wgrad_bf16x3(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows,
                                      const int32_t* group_off, int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, float* out,
                                      int64_t out_group_stride, float* colsum, int64_t colsum_group_stride, void* stream) {
    if (!A || !B || !rows || !group_off || !out || n_groups <= 0 || n_rows < 0 || m <= 0 || n_cols <= 0) return HGT_ERR_INVALID_ARG;
    if (n_rows == 0) return HGT_OK;
    const int n_mt = (m + WX_T - 1) / WX_T, n_nt = (n_cols + WX_T - 1) / WX_T;
    const int64_t chunks = (n_rows + WX_ROWS - 1) / WX_ROWS + n_groups;    // device-side group sizes: launch the upper bound
    if (chunks > 65535) return HGT_ERR_TOO_LARGE;
    dim3 grid((unsigned)(n_mt * n_nt), (unsigned)chunks);
    k_typed_wgrad_x3<<<grid, 256, 0, (hipStream_t)stream>>>(A, lda, B, ldb, rows, group_off, n_groups, m, n_cols, n_mt, out, out_group_stride,
                                                          colsum, colsum_group_stride);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_typed_colsum(const float* A, int64_t lda, const int32_t* rows, const int32_t* group_off, int32_t n_groups,
                                int64_t n_rows, int32_t m, float* out, int64_t out_group_stride, void* stream) {
    if (!A || !rows || !group_off || !out || n_groups <= 0 || n_rows < 0 || m <= 0) return HGT_ERR_INVALID_ARG;
    if (n_rows == 0) return HGT_OK;
    const int64_t waves = (n_rows + 255) / 256 + n_groups;
    k_typed_colsum<<<nblk(waves, 4), 256, 0, (hipStream_t)stream>>>(A, lda, rows, group_off, n_groups, m, out, out_group_stride);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_relation_outer(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad,
                                  const float* weights, const float* a_src, const float* rte_a, const float* b_dst, float* out,
                                  void* stream) {
    if (!plan || !a_src || !b_dst || !out || (E > 0 && !weights) || H <= 0 || 64 % H != 0 || dk_pad <= 0) return HGT_ERR_INVALID_ARG;
    if (E == 0) return HGT_OK;
    const int lph = 64 / H;
    if (dk_pad % lph != 0) return HGT_ERR_INVALID_ARG;
    HgtPlanView pv = hgt_plan_view(plan, N, E, T, R);
    // the per-lane accumulator block is VEC x DKP floats: split head groups until it fits 256 registers
    int vec = dk_pad / lph, l2 = lph;
    while (vec * dk_pad > 128 && vec > 1 && l2 * 2 <= 64) { vec /= 2; l2 *= 2; }
    int rc = dispatch_layout<LaunchOuter>(vec, l2, pv, weights, a_src, rte_a, b_dst, out, (int)R, (int)H, (hipStream_t)stream);
    if (rc != HGT_OK) return rc;
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

// hgt_relation_outer for heads of 128 / 256 padded columns (ABI 8): same arguments and contract (+= into the caller's buffer, a
// relation without edges stays untouched, rte_a optional).  Everything else is HGT_ERR_UNSUPPORTED and launches nothing:
// hgt_relation_outer keeps the narrower heads.
extern "C" int hgt_relation_outer_wide(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad,
                                       const float* weights, const float* a_src, const float* rte_a, const float* b_dst, float* out,
                                       void* stream) {
    if (!plan || !a_src || !b_dst || !out || (E > 0 && !weights) || H <= 0 || R <= 0 || dk_pad <= 0) return HGT_ERR_INVALID_ARG;
    if (dk_pad != 128 && dk_pad != 256) return HGT_ERR_UNSUPPORTED;
    if ((((uintptr_t)a_src | (uintptr_t)b_dst | (uintptr_t)rte_a) & 15) != 0) return HGT_ERR_INVALID_ARG;      // 16-byte row loads
    const int64_t blocks = (int64_t)H * (dk_pad / 128) * (dk_pad / 128);
    if (blocks > 65535 || R > 65535) return HGT_ERR_TOO_LARGE;
    if (E == 0) return HGT_OK;
    HgtPlanView pv = hgt_plan_view(plan, N, E, T, R);
    // items are ordered (tile, relation): ~8 / ~64 items of the selected relation per workgroup, the two regimes of LaunchOuter::run
    // (sampled batches: enough workgroups to fill the chip; large graphs: fewer 128 x 128 atomic flushes)
    const int ipw = (pv.L.max_items < 16384 ? OW_ITEMS_SMALL : OW_ITEMS_LARGE) * (R + 1);
    dim3 grid((unsigned)((pv.L.max_items + ipw - 1) / ipw), (unsigned)blocks, (unsigned)R);
    if (grid.x == 0) return HGT_OK;
    if (rte_a)
        k_relation_outer_wide<true><<<grid, 256, 0, (hipStream_t)stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, weights, a_src,
                                                                            rte_a, b_dst, out, (int)H, (int)dk_pad, ipw);
    else
        k_relation_outer_wide<false><<<grid, 256, 0, (hipStream_t)stream>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, weights, a_src,
                                                                             rte_a, b_dst, out, (int)H, (int)dk_pad, ipw);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

// =============================================================================================
// Deterministic forms (include/hgt_hip.h, "Bit-reproducible training").  Slot counts: pure functions of the
// arguments of the *_det_bytes calls.  DET_FLOOR: what every workspace may take on a small problem; large problems get a
// fraction of the bytes of the operands they read (which the caller holds anyway: the saved Q|K|V of the layer bounds them).
// =============================================================================================
namespace {

constexpr uint64_t DET_FLOOR = 32ull << 20;

// floats of a workspace of n_slots partials of n_elems floats, + the segment sums of the two-pass reduce
inline uint64_t det_ws_floats(int64_t n_slots, uint64_t n_elems) {
    return (uint64_t)n_slots * n_elems + (n_slots > DET_TWO_PASS ? (uint64_t)((n_slots + DET_SEG - 1) / DET_SEG) * n_elems : 0);
}
// the largest slot count <= want whose workspace fits `budget` bytes (at least 1)
inline int64_t det_fit_slots(int64_t want, uint64_t n_elems, uint64_t budget) {
    const uint64_t per = n_elems * 4;
    int64_t s = (int64_t)(budget / (per ? per : 1));
    if (s > DET_TWO_PASS) s = (int64_t)(budget / (per + per / DET_SEG + 1));      // the segment sums come on top
    if (s > want) s = want;
    return s < 1 ? 1 : s;
}

// out[(i / per) * ogs + i % per] = sum over the n_slots partials ([slot][slot_stride] floats, the first n_elems of each) in slot order;
// scratch: the segment sums (after the partials; only read when n_slots > DET_TWO_PASS)
void det_reduce(const float* part, int64_t n_slots, int64_t slot_stride, int64_t n_elems, float* scratch, float* out, int64_t per,
                int64_t ogs, hipStream_t stream) {
    if (n_elems <= 0) return;
    const unsigned bx = nblk(n_elems, 256);
    if (n_slots > DET_TWO_PASS) {
        const int nseg = (int)((n_slots + DET_SEG - 1) / DET_SEG);
        k_det_reduce<<<dim3(bx, (unsigned)nseg), 256, 0, stream>>>(part, (int)n_slots, slot_stride, n_elems, DET_SEG, scratch, n_elems, n_elems, n_elems);
        k_det_reduce<<<dim3(bx, 1), 256, 0, stream>>>(scratch, nseg, n_elems, n_elems, nseg, out, 0, per, ogs);
    } else {
        k_det_reduce<<<dim3(bx, 1), 256, 0, stream>>>(part, (int)n_slots, slot_stride, n_elems, (int)n_slots, out, 0, per, ogs);
    }
}

inline bool det_ws_bad(const void* ws, uint64_t need) { return need > 0 && (!ws || ((uintptr_t)ws & 15) != 0); }

// ---- node update: wavefronts = min(rows / 4, 4096, what DET_FLOOR holds), each a range of consecutive rows
struct DetNub { int64_t slots, rows_per_wave, slot_floats; };
inline DetNub det_nub(int64_t n_rows, int d, int T) {
    DetNub p;
    p.slot_floats = 2 * (int64_t)T * d + T;               // [T][d] d_ln_w | [T][d] d_ln_b | [T] d_alpha
    int64_t want = (n_rows + 3) / 4;
    if (want > 4096) want = 4096;
    const int64_t s = det_fit_slots(want < 1 ? 1 : want, (uint64_t)p.slot_floats, DET_FLOOR);
    p.rows_per_wave = n_rows > 0 ? (n_rows + s - 1) / s : 1;
    p.slots = n_rows > 0 ? (n_rows + p.rows_per_wave - 1) / p.rows_per_wave : 1;
    return p;
}

// ---- typed weight gradient: `chunks` row chunks per group; budget = max(DET_FLOOR, 1/16 of the bytes of A and B).  A slot holds the
// weight partials and (bf16 x3 form: with_colsum) the column-sum partials; chunks x groups stays inside the grid's y / x extent
inline int64_t det_wgrad_chunks(int n_groups, int64_t n_rows, int m, int n_cols, int64_t chunk_rows, bool with_colsum) {
    const uint64_t budget = max(DET_FLOOR, (uint64_t)n_rows * (uint64_t)(m + n_cols) * 4 / 16);
    int64_t want = (n_rows + chunk_rows - 1) / chunk_rows;
    if (want > 1024) want = 1024;
    if (want > 65535 / n_groups) want = 65535 / n_groups;
    return det_fit_slots(want < 1 ? 1 : want, (uint64_t)n_groups * m * (n_cols + (with_colsum ? 1 : 0)), budget);
}
// ---- column sums: chunks of >= 256 rows, at most 1024 per group, inside DET_FLOOR / 2
inline int64_t det_colsum_chunks(int n_groups, int64_t n_rows, int m) {
    int64_t want = (n_rows + 255) / 256;
    if (want > 1024) want = 1024;
    return det_fit_slots(want < 1 ? 1 : want, (uint64_t)n_groups * m, DET_FLOOR / 2);
}
inline uint64_t det_chunk_ws_floats(int64_t chunks, uint64_t elems) { return chunks > 1 ? det_ws_floats(chunks, elems) : 0; }

// ---- relation outer products: slices of the plan's item list; budget = max(DET_FLOOR, 1/4 of the bytes of Q|K|V)
struct DetOuter { int64_t slots; int ipw; uint64_t slot_floats; };
inline DetOuter det_outer(int64_t N, int64_t max_items, int R, int H, int dkp, bool wide) {
    DetOuter p;
    p.slot_floats = (uint64_t)R * H * dkp * dkp;
    const uint64_t budget = max(DET_FLOOR, (uint64_t)N * H * dkp * 4 * 3 / 4);
    const int ipw0 = wide ? (max_items < 16384 ? OW_ITEMS_SMALL : OW_ITEMS_LARGE) * (R + 1) : outer_items_per_wave(max_items, R);
    const int64_t want = max((int64_t)1, (max_items + ipw0 - 1) / ipw0);
    // (the narrow kernels launch whole workgroups of four wavefronts = four slots: four is the least they take, also where four
    //  partials pass the budget -- 4 R H dkp^2 floats, dkp <= 64: more than DET_FLOOR only from R H > 512 on)
    int64_t s = det_fit_slots(want + (wide ? 0 : 3), p.slot_floats, budget);
    if (!wide) s = max((int64_t)4, s / 4 * 4);
    const int64_t ipw = max((int64_t)ipw0, (max_items + s - 1) / s);
    p.ipw = (int)ipw;
    const int64_t used = max((int64_t)1, (max_items + ipw - 1) / ipw);
    p.slots = wide ? used : (used + 3) / 4 * 4;
    return p;
}

}  // namespace

extern "C" int hgt_node_update_bwd_det_bytes(int64_t n_rows, int32_t d, int32_t n_types, uint64_t* out) {
    if (!out || n_rows < 0 || d <= 0 || d > 64 * NUB_MAXC_WIDE || n_types <= 0) return HGT_ERR_INVALID_ARG;
    const DetNub p = det_nub(n_rows, d, n_types);
    *out = n_rows == 0 ? 0 : det_ws_floats(p.slots, (uint64_t)p.slot_floats) * 4;
    return HGT_OK;
}

extern "C" int hgt_node_update_bwd_det(const float* grad_out, const float* trans, const float* x, int64_t ldx, const int64_t* node_type,
                                       const float* skip, const float* ln_w, int32_t use_norm, int32_t shared_norm, const float* drop_mask,
                                       int64_t n_rows, int32_t d, int32_t n_types, float* d_trans, float* dx, int64_t ld_dx,
                                       float* d_alpha, float* d_ln_w, float* d_ln_b, void* ws, uint64_t ws_bytes, void* stream) {
    if (!grad_out || !trans || !x || !node_type || !d_trans || !dx || (skip && !d_alpha) || n_rows < 0 || d <= 0 ||
        d > 64 * NUB_MAXC_WIDE || n_types <= 0)
        return HGT_ERR_INVALID_ARG;
    if (use_norm && (!ln_w || !d_ln_w || !d_ln_b)) return HGT_ERR_INVALID_ARG;
    uint64_t need = 0;
    hgt_node_update_bwd_det_bytes(n_rows, d, n_types, &need);
    if (det_ws_bad(ws, need)) return HGT_ERR_INVALID_ARG;
    if (ws_bytes < need) return HGT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t ln_elems = (int64_t)(shared_norm ? 1 : n_types) * d;
    if (n_rows == 0) {      // overwritten outputs: zeros
        if (use_norm) { (void)hipMemsetAsync(d_ln_w, 0, ln_elems * 4, st); (void)hipMemsetAsync(d_ln_b, 0, ln_elems * 4, st); }
        if (skip) (void)hipMemsetAsync(d_alpha, 0, (size_t)n_types * 4, st);
        HGT_CHECK_LAUNCH();
        return HGT_OK;
    }
    const DetNub p = det_nub(n_rows, d, n_types);
    float* part = (float*)ws;
    float* scratch = part + p.slots * p.slot_floats;
    const int64_t td = (int64_t)n_types * d;
    (void)hipMemsetAsync(part, 0, (size_t)(p.slots * p.slot_floats) * 4, st);      // a wavefront adds to its slot once per run of one type
    auto* kernel = d <= 64 * NUB_MAXC ? k_det_node_update_bwd : k_det_node_update_bwd_wide;
    kernel<<<nblk(p.slots, 4), 256, 0, st>>>(grad_out, trans, x, ldx, node_type, skip, ln_w, use_norm, drop_mask, n_rows, d, n_types, d_trans,
                                            dx, ld_dx, skip ? part + 2 * td : nullptr, use_norm ? part : nullptr,
                                            use_norm ? part + td : nullptr, shared_norm, (int)p.rows_per_wave, p.slot_floats);
    if (use_norm) {
        det_reduce(part, p.slots, p.slot_floats, ln_elems, scratch, d_ln_w, ln_elems, ln_elems, st);
        det_reduce(part + td, p.slots, p.slot_floats, ln_elems, scratch, d_ln_b, ln_elems, ln_elems, st);
    }
    if (skip) det_reduce(part + 2 * td, p.slots, p.slot_floats, n_types, scratch, d_alpha, n_types, n_types, st);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

// zero the [n_groups][per] blocks of a grouped output (group stride ogs floats)
static void det_zero_groups(float* out, int n_groups, int64_t per, int64_t ogs, hipStream_t st) {
    (void)hipMemset2DAsync(out, (size_t)ogs * 4, 0, (size_t)per * 4, (size_t)n_groups, st);
}

extern "C" int hgt_typed_wgrad_det_bytes(int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, uint64_t* out) {
    if (!out || n_groups <= 0 || n_rows < 0 || m <= 0 || n_cols <= 0) return HGT_ERR_INVALID_ARG;
    if (n_groups > 65535) return HGT_ERR_TOO_LARGE;
    *out = det_chunk_ws_floats(det_wgrad_chunks(n_groups, n_rows, m, n_cols, WG_ROWS, false), (uint64_t)n_groups * m * n_cols) * 4;
    return HGT_OK;
}

extern "C" int hgt_typed_wgrad_det(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows,
                                   const int32_t* group_off, int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, float* out,
                                   int64_t out_group_stride, void* ws, uint64_t ws_bytes, void* stream) {
    if (!A || !B || !rows || !group_off || !out || n_groups <= 0 || n_rows < 0 || m <= 0 || n_cols <= 0 ||
        out_group_stride < (int64_t)m * n_cols)
        return HGT_ERR_INVALID_ARG;
    uint64_t need = 0;
    int rcb = hgt_typed_wgrad_det_bytes(n_groups, n_rows, m, n_cols, &need);
    if (rcb != HGT_OK) return rcb;
    if (det_ws_bad(ws, need)) return HGT_ERR_INVALID_ARG;
    if (ws_bytes < need) return HGT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t per = (int64_t)m * n_cols, elems = per * n_groups;
    if (n_rows == 0) { det_zero_groups(out, n_groups, per, out_group_stride, st); HGT_CHECK_LAUNCH(); return HGT_OK; }
    const int64_t chunks = det_wgrad_chunks(n_groups, n_rows, m, n_cols, WG_ROWS, false);
    const int vecA = ((lda & 3) == 0 && ((uintptr_t)A & 15) == 0), vecB = ((ldb & 3) == 0 && ((uintptr_t)B & 15) == 0);
    float* part = chunks > 1 ? (float*)ws : out;
    dim3 grid((unsigned)(chunks * n_groups), (unsigned)((m + 63) / 64), (unsigned)((n_cols + 63) / 64));
    k_det_typed_wgrad<<<grid, 256, 0, st>>>(A, lda, B, ldb, rows, group_off, n_groups, m, n_cols, part, chunks > 1 ? per : out_group_stride,
                                           vecA, vecB, (int)chunks);
    if (chunks > 1) det_reduce(part, chunks, elems, elems, part + chunks * elems, out, per, out_group_stride, st);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_typed_wgrad_bf16x3_det_bytes(int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols, uint64_t* out) {
    if (!out || n_groups <= 0 || n_rows < 0 || m <= 0 || n_cols <= 0) return HGT_ERR_INVALID_ARG;
    if (n_groups > 65535) return HGT_ERR_TOO_LARGE;
    const int64_t chunks = det_wgrad_chunks(n_groups, n_rows, m, n_cols, WX_ROWS, true);
    // the weight partials, then the column-sum partials (always provided for: the size does not depend on the colsum argument)
    *out = (det_chunk_ws_floats(chunks, (uint64_t)n_groups * m * n_cols) + det_chunk_ws_floats(chunks, (uint64_t)n_groups * m)) * 4;
    return HGT_OK;
}

extern "C" int hgt_typed_wgrad_bf16x3_det(const float* A, int64_t lda, const float* B, int64_t ldb, const int32_t* rows,
                                          const int32_t* group_off, int32_t n_groups, int64_t n_rows, int32_t m, int32_t n_cols,
                                          float* out, int64_t out_group_stride, float* colsum, int64_t colsum_group_stride, void* ws,
                                          uint64_t ws_bytes, void* stream) {
    if (!A || !B || !rows || !group_off || !out || n_groups <= 0 || n_rows < 0 || m <= 0 || n_cols <= 0 ||
        out_group_stride < (int64_t)m * n_cols || (colsum && colsum_group_stride < m))
        return HGT_ERR_INVALID_ARG;
    uint64_t need = 0;
    int rcb = hgt_typed_wgrad_bf16x3_det_bytes(n_groups, n_rows, m, n_cols, &need);
    if (rcb != HGT_OK) return rcb;
    if (det_ws_bad(ws, need)) return HGT_ERR_INVALID_ARG;
    if (ws_bytes < need) return HGT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t per = (int64_t)m * n_cols, elems = per * n_groups, cs_elems = (int64_t)m * n_groups;
    if (n_rows == 0) {
        det_zero_groups(out, n_groups, per, out_group_stride, st);
        if (colsum) det_zero_groups(colsum, n_groups, m, colsum_group_stride, st);
        HGT_CHECK_LAUNCH();
        return HGT_OK;
    }
    const int64_t chunks = det_wgrad_chunks(n_groups, n_rows, m, n_cols, WX_ROWS, true);
    const int n_mt = (m + WX_T - 1) / WX_T, n_nt = (n_cols + WX_T - 1) / WX_T;
    float* part = chunks > 1 ? (float*)ws : out;
    float* cs_part = chunks > 1 ? (float*)ws + det_ws_floats(chunks, (uint64_t)elems) : colsum;
    dim3 grid((unsigned)(n_mt * n_nt), (unsigned)(chunks * n_groups));
    k_det_typed_wgrad_x3<<<grid, 256, 0, st>>>(A, lda, B, ldb, rows, group_off, n_groups, m, n_cols, n_mt, part,
                                              chunks > 1 ? per : out_group_stride, colsum ? cs_part : nullptr,
                                              chunks > 1 ? (int64_t)m : colsum_group_stride, (int)chunks);
    if (chunks > 1) {
        det_reduce(part, chunks, elems, elems, part + chunks * elems, out, per, out_group_stride, st);
        if (colsum) det_reduce(cs_part, chunks, cs_elems, cs_elems, cs_part + chunks * cs_elems, colsum, m, colsum_group_stride, st);
    }
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_typed_colsum_det_bytes(int32_t n_groups, int64_t n_rows, int32_t m, uint64_t* out) {
    if (!out || n_groups <= 0 || n_rows < 0 || m <= 0) return HGT_ERR_INVALID_ARG;
    *out = det_chunk_ws_floats(det_colsum_chunks(n_groups, n_rows, m), (uint64_t)n_groups * m) * 4;
    return HGT_OK;
}

extern "C" int hgt_typed_colsum_det(const float* A, int64_t lda, const int32_t* rows, const int32_t* group_off, int32_t n_groups,
                                    int64_t n_rows, int32_t m, float* out, int64_t out_group_stride, void* ws, uint64_t ws_bytes,
                                    void* stream) {
    if (!A || !rows || !group_off || !out || n_groups <= 0 || n_rows < 0 || m <= 0 || out_group_stride < m) return HGT_ERR_INVALID_ARG;
    uint64_t need = 0;
    hgt_typed_colsum_det_bytes(n_groups, n_rows, m, &need);
    if (det_ws_bad(ws, need)) return HGT_ERR_INVALID_ARG;
    if (ws_bytes < need) return HGT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) { det_zero_groups(out, n_groups, m, out_group_stride, st); HGT_CHECK_LAUNCH(); return HGT_OK; }
    const int64_t chunks = det_colsum_chunks(n_groups, n_rows, m), elems = (int64_t)m * n_groups;
    float* part = chunks > 1 ? (float*)ws : out;
    k_det_typed_colsum<<<nblk(chunks * n_groups, 4), 256, 0, st>>>(A, lda, rows, group_off, n_groups, m, part,
                                                                   chunks > 1 ? (int64_t)m : out_group_stride, (int)chunks);
    if (chunks > 1) det_reduce(part, chunks, elems, elems, part + chunks * elems, out, m, out_group_stride, st);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

static int outer_det_bytes(bool wide, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad, uint64_t* out) {
    if (!out || N < 0 || E < 0 || T <= 0 || R <= 0 || H <= 0 || dk_pad <= 0) return HGT_ERR_INVALID_ARG;
    if (wide ? (dk_pad != 128 && dk_pad != 256) : (64 % H != 0 || dk_pad % (64 / H) != 0)) return wide ? HGT_ERR_UNSUPPORTED : HGT_ERR_INVALID_ARG;
    if (E == 0) { *out = 0; return HGT_OK; }
    const DetOuter p = det_outer(N, hgt_plan_layout(N, E, T, R).max_items, R, H, dk_pad, wide);
    *out = det_ws_floats(p.slots, p.slot_floats) * 4;
    return HGT_OK;
}
extern "C" int hgt_relation_outer_det_bytes(int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad, uint64_t* out) {
    return outer_det_bytes(false, N, E, T, R, H, dk_pad, out);
}
extern "C" int hgt_relation_outer_wide_det_bytes(int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad, uint64_t* out) {
    return outer_det_bytes(true, N, E, T, R, H, dk_pad, out);
}

extern "C" int hgt_relation_outer_det(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad,
                                      const float* weights, const float* a_src, const float* rte_a, const float* b_dst, float* out,
                                      void* ws, uint64_t ws_bytes, void* stream) {
    if (!plan || !a_src || !b_dst || !out || (E > 0 && !weights) || H <= 0 || R <= 0 || 64 % H != 0 || dk_pad <= 0) return HGT_ERR_INVALID_ARG;
    const int lph = 64 / H;
    if (dk_pad % lph != 0) return HGT_ERR_INVALID_ARG;
    uint64_t need = 0;
    int rc = outer_det_bytes(false, N, E, T, R, H, dk_pad, &need);
    if (rc != HGT_OK) return rc;
    if (det_ws_bad(ws, need)) return HGT_ERR_INVALID_ARG;
    if (ws_bytes < need) return HGT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t elems = (int64_t)R * H * dk_pad * dk_pad;
    if (E == 0) { (void)hipMemsetAsync(out, 0, (size_t)elems * 4, st); HGT_CHECK_LAUNCH(); return HGT_OK; }
    HgtPlanView pv = hgt_plan_view(plan, N, E, T, R);
    const DetOuter p = det_outer(N, pv.L.max_items, R, H, dk_pad, false);
    int vec = dk_pad / lph, l2 = lph;
    while (vec * dk_pad > 128 && vec > 1 && l2 * 2 <= 64) { vec /= 2; l2 *= 2; }
    float* part = (float*)ws;
    rc = dispatch_layout<LaunchOuter>(vec, l2, pv, weights, a_src, rte_a, b_dst, part, (int)R, (int)H, st, p.ipw);
    if (rc != HGT_OK) return rc;
    det_reduce(part, p.slots, elems, elems, part + p.slots * elems, out, elems, elems, st);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_relation_outer_wide_det(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, int32_t dk_pad,
                                           const float* weights, const float* a_src, const float* rte_a, const float* b_dst, float* out,
                                           void* ws, uint64_t ws_bytes, void* stream) {
    if (!plan || !a_src || !b_dst || !out || (E > 0 && !weights) || H <= 0 || R <= 0 || dk_pad <= 0) return HGT_ERR_INVALID_ARG;
    if (dk_pad != 128 && dk_pad != 256) return HGT_ERR_UNSUPPORTED;
    if ((((uintptr_t)a_src | (uintptr_t)b_dst | (uintptr_t)rte_a) & 15) != 0) return HGT_ERR_INVALID_ARG;      // 16-byte row loads
    const int64_t blocks = (int64_t)H * (dk_pad / 128) * (dk_pad / 128);
    if (blocks > 65535 || R > 65535) return HGT_ERR_TOO_LARGE;
    uint64_t need = 0;
    int rc = outer_det_bytes(true, N, E, T, R, H, dk_pad, &need);
    if (rc != HGT_OK) return rc;
    if (det_ws_bad(ws, need)) return HGT_ERR_INVALID_ARG;
    if (ws_bytes < need) return HGT_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t elems = (int64_t)R * H * dk_pad * dk_pad;
    if (E == 0) { (void)hipMemsetAsync(out, 0, (size_t)elems * 4, st); HGT_CHECK_LAUNCH(); return HGT_OK; }
    HgtPlanView pv = hgt_plan_view(plan, N, E, T, R);
    const DetOuter p = det_outer(N, pv.L.max_items, R, H, dk_pad, true);
    float* part = (float*)ws;
    dim3 grid((unsigned)p.slots, (unsigned)blocks, (unsigned)R);
    if (rte_a)
        k_det_relation_outer_wide<true><<<grid, 256, 0, st>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, weights, a_src, rte_a, b_dst,
                                                             part, (int)H, (int)dk_pad, p.ipw);
    else
        k_det_relation_outer_wide<false><<<grid, 256, 0, st>>>(pv.items, pv.hdr, pv.esrc, pv.edst, pv.ertei, weights, a_src, rte_a, b_dst,
                                                              part, (int)H, (int)dk_pad, p.ipw);
    det_reduce(part, p.slots, elems, elems, part + p.slots * elems, out, elems, elems, st);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}
