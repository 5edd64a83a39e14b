// Backward pass of HGTConv: the kernels that have no forward counterpart -- this file: the node update and
// the element-wise helpers; hgt_bwd_wgrad.hip: the typed weight gradients; hgt_bwd_outer.hip: the relation outer products.  The reference gets its
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
// list, all fixed on the host from the problem sizes (the det_* plan functions next to each step's host function; hgt_det.h) -- and
// k_det_reduce sums the slots in slot order.  No atomics, no waiting between workgroups: two launches on the stream are the ordering.
#include "hgt_det.h"

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

// ---- launch geometry of the node update: wavefronts (= workspace slots of the det form), each a range of consecutive rows
struct NubPlan { int64_t slots, rows_per_wave; };
// atomic form: 32 rows per wavefront amortise the parameter-gradient atomics on a large graph; a sampled batch of a few thousand rows
// would be ~100 wavefronts walking 32 rows one after the other (c3: 119 us) -- 2 rows there, 8 in between
inline NubPlan nub_plan(int64_t n_rows) {
    const int rpw = n_rows >= 65536 ? NUB_ROWS : (n_rows >= 16384 ? 8 : 2);
    return {(n_rows + rpw - 1) / rpw, rpw};
}
// det form: slots = min(rows / 4, 4096, what DET_FLOOR holds) partials of [T][d] d_ln_w | [T][d] d_ln_b | [T] d_alpha
inline int64_t nub_slot_floats(int d, int T) { return 2 * (int64_t)T * d + T; }
inline NubPlan det_nub_plan(int64_t n_rows, int d, int T) {
    int64_t want = (n_rows + 3) / 4;
    if (want > 4096) want = 4096;
    const int64_t s = det_fit_slots(want < 1 ? 1 : want, (uint64_t)nub_slot_floats(d, T), DET_FLOOR);
    const int64_t rpw = n_rows > 0 ? (n_rows + s - 1) / s : 1;
    return {n_rows > 0 ? (n_rows + rpw - 1) / rpw : 1, rpw};
}

inline bool nub_sizes_bad(int64_t n_rows, int32_t d) { return n_rows < 0 || d <= 0 || d > 64 * NUB_MAXC_WIDE; }

}  // namespace

extern "C" int hgt_node_update_bwd_det_bytes(int64_t n_rows, int32_t d, int32_t n_types, uint64_t* out) {
    if (!out || nub_sizes_bad(n_rows, d) || n_types <= 0) return HGT_ERR_INVALID_ARG;
    *out = n_rows == 0 ? 0 : det_ws_floats(det_nub_plan(n_rows, d, n_types).slots, (uint64_t)nub_slot_floats(d, n_types)) * 4;
    return HGT_OK;
}

// the arguments of the entry points in front of and behind `shared_norm` (hgt_node_update_bwd has none)
#define HGT_NUB_HEAD_PARAMS                                                                                                          \
    const float *grad_out, const float *trans, const float *x, int64_t ldx, const int64_t *node_type, const float *skip,            \
        const float *ln_w, int32_t use_norm
#define HGT_NUB_HEAD_ARGS grad_out, trans, x, ldx, node_type, skip, ln_w, use_norm
#define HGT_NUB_TAIL_PARAMS                                                                                                          \
    const float *drop_mask, int64_t n_rows, int32_t d, int32_t n_types, float *d_trans, float *dx, int64_t ld_dx, float *d_alpha,   \
        float *d_ln_w, float *d_ln_b
#define HGT_NUB_TAIL_ARGS drop_mask, n_rows, d, n_types, d_trans, dx, ld_dx, d_alpha, d_ln_w, d_ln_b

// hgt_node_update_bwd[_ex] (det == NULL) and hgt_node_update_bwd_det.  skip == NULL = plain residual (no gate, d_alpha unused),
// shared_norm = one LayerNorm for all types.  (Only the det form needs n_types > 0: it sizes its slots with it.)
static int node_update_bwd_impl(HGT_NUB_HEAD_PARAMS, int32_t shared_norm, HGT_NUB_TAIL_PARAMS, const HgtDetWs* det, void* stream) {
    if (!grad_out || !trans || !x || !node_type || !d_trans || !dx || (skip && !d_alpha) || nub_sizes_bad(n_rows, d) ||
        (det && n_types <= 0))
        return HGT_ERR_INVALID_ARG;
    if (use_norm && (!ln_w || !d_ln_w || !d_ln_b)) return HGT_ERR_INVALID_ARG;
    if (det) {
        uint64_t need = 0;
        hgt_node_update_bwd_det_bytes(n_rows, d, n_types, &need);
        if (int rc = det_ws_check(*det, need)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t ln_elems = (int64_t)(shared_norm ? 1 : n_types) * d;
    if (n_rows == 0) {
        if (!det) return HGT_OK;
        // overwritten outputs: zeros
        if (use_norm) { (void)hipMemsetAsync(d_ln_w, 0, ln_elems * 4, st); (void)hipMemsetAsync(d_ln_b, 0, ln_elems * 4, st); }
        if (skip) (void)hipMemsetAsync(d_alpha, 0, (size_t)n_types * 4, st);
        HGT_CHECK_LAUNCH();
        return HGT_OK;
    }
    const NubPlan p = det ? det_nub_plan(n_rows, d, n_types) : nub_plan(n_rows);
    // d <= 512 keeps the 8-columns-per-lane kernel (its registers, its results); wider rows take the 16-column instantiation
    const bool wide = d > 64 * NUB_MAXC;
    if (det) {
        const int64_t slot_floats = nub_slot_floats(d, n_types), td = (int64_t)n_types * d;
        float* part = (float*)det->ptr;
        float* scratch = part + p.slots * slot_floats;
        (void)hipMemsetAsync(part, 0, (size_t)(p.slots * slot_floats) * 4, st);      // a wavefront adds to its slot once per run of one type
        auto* kernel = wide ? k_det_node_update_bwd_wide : k_det_node_update_bwd;
        kernel<<<nblk(p.slots, 4), 256, 0, st>>>(grad_out, trans, x, ldx, node_type, skip, ln_w, use_norm, drop_mask, n_rows, d, n_types,
                                                d_trans, dx, ld_dx, skip ? part + 2 * td : nullptr, use_norm ? part : nullptr,
                                                use_norm ? part + td : nullptr, shared_norm, (int)p.rows_per_wave, slot_floats);
        if (use_norm) {
            det_reduce(part, p.slots, slot_floats, ln_elems, scratch, d_ln_w, ln_elems, ln_elems, st);
            det_reduce(part + td, p.slots, slot_floats, ln_elems, scratch, d_ln_b, ln_elems, ln_elems, st);
        }
        if (skip) det_reduce(part + 2 * td, p.slots, slot_floats, n_types, scratch, d_alpha, n_types, n_types, st);
    } else {
        auto* kernel = wide ? k_node_update_bwd_wide : k_node_update_bwd;
        kernel<<<nblk(p.slots, 4), 256, 0, st>>>(grad_out, trans, x, ldx, node_type, skip, ln_w, use_norm, drop_mask, n_rows, d, n_types,
                                                d_trans, dx, ld_dx, d_alpha, d_ln_w, d_ln_b, shared_norm, (int)p.rows_per_wave);
    }
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

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

extern "C" int hgt_node_update_bwd(HGT_NUB_HEAD_PARAMS, HGT_NUB_TAIL_PARAMS, void* stream) {
    if (!skip) return HGT_ERR_INVALID_ARG;
    return node_update_bwd_impl(HGT_NUB_HEAD_ARGS, 0, HGT_NUB_TAIL_ARGS, nullptr, stream);
}
// reverse of hgt_node_update_ex
extern "C" int hgt_node_update_bwd_ex(HGT_NUB_HEAD_PARAMS, int32_t shared_norm, HGT_NUB_TAIL_PARAMS, void* stream) {
    return node_update_bwd_impl(HGT_NUB_HEAD_ARGS, shared_norm, HGT_NUB_TAIL_ARGS, nullptr, stream);
}
extern "C" int hgt_node_update_bwd_det(HGT_NUB_HEAD_PARAMS, int32_t shared_norm, HGT_NUB_TAIL_PARAMS, void* ws, uint64_t ws_bytes,
                                       void* stream) {
    const HgtDetWs det = {ws, ws_bytes};
    return node_update_bwd_impl(HGT_NUB_HEAD_ARGS, shared_norm, HGT_NUB_TAIL_ARGS, &det, stream);
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
    // E == 0: the per-edge arrays att / d_att / d_logits may be NULL (rho is per node)
    if (!plan || !rho || (E > 0 && (!att || !d_att || !d_logits)) || H <= 0) return HGT_ERR_INVALID_ARG;
    if (E == 0) return HGT_OK;
    HgtPlanView pv = hgt_plan_view(plan, N, E, T, R);
    k_edge_softmax_bwd<<<nblk(E * H, 256), 256, 0, (hipStream_t)stream>>>(pv.edst, att, d_att, rho, ld_rho, d_logits, E, H);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_edge_gather_sorted(const void* plan, int64_t N, int64_t E, int32_t T, int32_t R, int32_t H, const float* by_edge_id,
                                      float* sorted, void* stream) {
    if (!plan || (E > 0 && (!by_edge_id || !sorted)) || H <= 0) return HGT_ERR_INVALID_ARG;      // E == 0: both may be NULL
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
