// The optimizer step of a training script on the device (gfx950): what every script of the reference ends a step with,
//   torch.nn.utils.clip_grad_norm_(model.parameters(), clip); optimizer.step()          (OAG/train_paper_field.py:251-252)
// with optimizer = torch.optim.AdamW -- over a model of 50-200 small tensors, in three launches whatever the number of tensors.
//
//   hgt_grad_sqnorm      a workgroup per chunk (at most HGT_OPTIM_CHUNK elements of one tensor): the fp64 sum of the squares of its
//                        gradient elements into partials[chunk]; 0 for a tensor without a gradient or of a group with clip off
//   hgt_grad_norm_join   one workgroup: total_norm = (float)sqrt(sum of the partials)
//   hgt_adamw_step       a workgroup per chunk: coef = min(1, max_norm / (total_norm + 1e-6f)) as clip_grad_norm_ forms it, then per
//                        element, in fp32 and in the order of torch/optim/adamw.py (single-tensor form):
//                          g *= coef (clipped groups);  g = -g (maximize);  p *= 1 - lr wd;  m = b1 m + (1 - b1) g;
//                          v = b2 v + (1 - b2) g g;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
//                        bc1 = 1 - b1^step, bc2 = 1 - b2^step and the scalars derived from them are formed in fp64, once per workgroup.
//                        p, m and v are written; the gradient is not.
//
// Summation order.  Thread t of a chunk's workgroup owns the quads t, t + 256, ... of the chunk, whether they are read with one 16-byte
// load or four scalar ones; it adds their squares in fp64 in element order, the 64 sums of a wavefront are joined by a shuffle tree,
// the wavefronts one after the other.  The join adds partials t, t + 256, ... per thread and ends in the same tree.  No atomics: the
// bits of total_norm depend on the gradients and the chunk table alone, and every workgroup of the update reads the same float.
// Every product and sum of the update is written as an explicit fmaf / single operation, so the two access paths cannot be contracted
// differently: element i of a tensor gets the same bits on either.  Compiled without fast-math like the rest of the library.
#include <limits.h>
#include <math.h>

#include "hgt_common.h"

namespace {

constexpr int OPT_BLOCK = 256;
constexpr int OPT_WAVES = OPT_BLOCK / 64;
constexpr int OPT_QUADS = HGT_OPTIM_CHUNK / (4 * OPT_BLOCK);       // quads a thread owns in a full chunk
static_assert(HGT_OPTIM_CHUNK % (4 * OPT_BLOCK) == 0, "a chunk is a whole number of quads per thread");
static_assert(sizeof(hgt_optim_tensor) == 64 && sizeof(hgt_optim_group) == 64 && sizeof(hgt_optim_chunk) == 16, "table rows");

struct OptArgs {
    const hgt_optim_tensor* tensors;
    const hgt_optim_group* groups;
    const hgt_optim_chunk* chunks;
    double* partials;
    const float* total_norm;
    float max_norm;
    int32_t n_tensors, n_groups;
};

// the row of a chunk, or false where the tables do not name a tensor with a gradient (nothing is read through such a row)
__device__ __forceinline__ bool chunk_row(const OptArgs& A, hgt_optim_chunk& c, hgt_optim_tensor& t, hgt_optim_group& g) {
    c = A.chunks[blockIdx.x];
    if (c.row < 0 || c.row >= A.n_tensors) return false;
    t = A.tensors[c.row];
    if (!t.p || !t.g || !t.exp_avg || !t.exp_avg_sq || t.group < 0 || t.group >= A.n_groups) return false;
    if (c.first < 0 || c.first >= t.numel) return false;
    g = A.groups[t.group];
    return true;
}

__device__ __forceinline__ double block_sum(double v, double* lds) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    v = lds[0];
    for (int q = 1; q < OPT_WAVES; ++q) v += lds[q];
    return v;
}

__global__ void __launch_bounds__(OPT_BLOCK) k_grad_sqnorm(OptArgs A) {
    __shared__ double lds[OPT_WAVES];
    hgt_optim_chunk c;
    hgt_optim_tensor t;
    hgt_optim_group grp;
    if (!chunk_row(A, c, t, grp) || !grp.clip) {                                  // uniform over the workgroup
        if (threadIdx.x == 0) A.partials[blockIdx.x] = 0.0;
        return;
    }
    const float* g = (const float*)t.g;
    const int64_t end = t.numel - c.first < HGT_OPTIM_CHUNK ? t.numel : c.first + HGT_OPTIM_CHUNK;
    const bool vec = t.aligned && (c.first & 3) == 0;                             // a foreign table's chunk may start off a quad
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < OPT_QUADS; ++k) {
        const int64_t e = c.first + 4 * ((int64_t)threadIdx.x + (int64_t)OPT_BLOCK * k);
        if (vec && e + 3 < end) {
            const float4 q = *reinterpret_cast<const float4*>(g + e);
            acc += (double)q.x * (double)q.x;
            acc += (double)q.y * (double)q.y;
            acc += (double)q.z * (double)q.z;
            acc += (double)q.w * (double)q.w;
        } else {
            for (int j = 0; j < 4; ++j) {
                if (e + j < end) acc += (double)g[e + j] * (double)g[e + j];
            }
        }
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) A.partials[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(OPT_BLOCK) k_grad_norm_join(const double* partials, int64_t n, float* total_norm) {
    __shared__ double lds[OPT_WAVES];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += OPT_BLOCK) acc += partials[i];
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) *total_norm = (float)sqrt(acc);
}

struct Scalars {
    float coef, decay, b1, omb1, b2, omb2, step_size, bc2_sqrt, eps;
    bool clip, maximize;
};

__device__ __forceinline__ void update_one(const Scalars& S, float g, float& p, float& m, float& v) {
    if (S.clip) g = g * S.coef;
    if (S.maximize) g = -g;
    p = p * S.decay;
    m = fmaf(S.omb1, g, S.b1 * m);
    v = fmaf(S.omb2 * g, g, S.b2 * v);
    const float denom = sqrtf(v) / S.bc2_sqrt + S.eps;
    p = fmaf(-S.step_size, m / denom, p);
}

__global__ void __launch_bounds__(OPT_BLOCK) k_adamw_step(OptArgs A) {
    hgt_optim_chunk c;
    hgt_optim_tensor t;
    hgt_optim_group grp;
    if (!chunk_row(A, c, t, grp)) return;                                         // uniform over the workgroup
    Scalars S;
    S.clip = A.total_norm != nullptr && grp.clip != 0;
    S.maximize = grp.maximize != 0;
    S.coef = 1.0f;
    if (S.clip) {
        const float coef = A.max_norm / (*A.total_norm + 1e-6f);
        S.coef = coef > 1.0f ? 1.0f : coef;                                       // a NaN stays a NaN, as in torch.clamp(max=1)
    }
    const double bc1 = 1.0 - pow(grp.beta1, (double)t.step), bc2 = 1.0 - pow(grp.beta2, (double)t.step);
    S.decay = (float)(1.0 - grp.lr * grp.weight_decay);
    S.b1 = (float)grp.beta1, S.omb1 = (float)(1.0 - grp.beta1);
    S.b2 = (float)grp.beta2, S.omb2 = (float)(1.0 - grp.beta2);
    S.step_size = (float)(grp.lr / bc1);
    S.bc2_sqrt = (float)sqrt(bc2);
    S.eps = (float)grp.eps;

    float* p = (float*)t.p;
    const float* g = (const float*)t.g;
    float* m = (float*)t.exp_avg;
    float* v = (float*)t.exp_avg_sq;
    const int64_t end = t.numel - c.first < HGT_OPTIM_CHUNK ? t.numel : c.first + HGT_OPTIM_CHUNK;
    const bool vec = t.aligned && (c.first & 3) == 0;
#pragma unroll
    for (int k = 0; k < OPT_QUADS; ++k) {
        const int64_t e = c.first + 4 * ((int64_t)threadIdx.x + (int64_t)OPT_BLOCK * k);
        if (vec && e + 3 < end) {
            float4 pq = *reinterpret_cast<const float4*>(p + e), mq = *reinterpret_cast<const float4*>(m + e);
            float4 vq = *reinterpret_cast<const float4*>(v + e);
            const float4 gq = *reinterpret_cast<const float4*>(g + e);
            update_one(S, gq.x, pq.x, mq.x, vq.x);
            update_one(S, gq.y, pq.y, mq.y, vq.y);
            update_one(S, gq.z, pq.z, mq.z, vq.z);
            update_one(S, gq.w, pq.w, mq.w, vq.w);
            *reinterpret_cast<float4*>(p + e) = pq;
            *reinterpret_cast<float4*>(m + e) = mq;
            *reinterpret_cast<float4*>(v + e) = vq;
        } else {
            for (int j = 0; j < 4; ++j) {
                if (e + j < end) update_one(S, g[e + j], p[e + j], m[e + j], v[e + j]);
            }
        }
    }
}

int optim_args_ok(const hgt_optim_tensor* tensors, int32_t n_tensors, const hgt_optim_group* groups, int32_t n_groups,
                  const hgt_optim_chunk* chunks, int64_t n_chunks) {
    if (n_tensors < 0 || n_groups < 0 || n_chunks < 0) return HGT_ERR_INVALID_ARG;
    if (n_chunks == 0) return HGT_OK;
    if (n_tensors < 1 || n_groups < 1 || !tensors || !groups || !chunks) return HGT_ERR_INVALID_ARG;
    if (n_chunks > INT_MAX) return HGT_ERR_UNSUPPORTED;                            // a workgroup per chunk, one grid dimension
    return HGT_OK;
}

}  // namespace

extern "C" int hgt_optim_constants(int32_t* chunk_host) {
    if (!chunk_host) return HGT_ERR_INVALID_ARG;
    *chunk_host = HGT_OPTIM_CHUNK;
    return HGT_OK;
}

extern "C" int hgt_optim_chunk_table(const int64_t* numel_host, int32_t n_tensors, hgt_optim_chunk* chunks_host, int64_t capacity,
                                     int64_t* n_chunks_host) {
    if (n_tensors < 0 || capacity < 0 || !n_chunks_host || (n_tensors > 0 && !numel_host)) return HGT_ERR_INVALID_ARG;
    int64_t n = 0;
    for (int32_t r = 0; r < n_tensors; ++r) {
        if (numel_host[r] < 0) return HGT_ERR_INVALID_ARG;
        const int64_t per = numel_host[r] / HGT_OPTIM_CHUNK + (numel_host[r] % HGT_OPTIM_CHUNK != 0);
        if (per > INT_MAX - n) {
            *n_chunks_host = 0;
            return HGT_ERR_UNSUPPORTED;
        }
        n += per;
    }
    *n_chunks_host = n;
    if (!chunks_host) return HGT_OK;                                              // the size query
    if (capacity < n) return HGT_ERR_WORKSPACE;
    int64_t c = 0;
    for (int32_t r = 0; r < n_tensors; ++r) {
        for (int64_t first = 0; first < numel_host[r]; first += HGT_OPTIM_CHUNK, ++c) {
            chunks_host[c].first = first;
            chunks_host[c].row = r;
            chunks_host[c].reserved = 0;
        }
    }
    return HGT_OK;
}

extern "C" int hgt_optim_tables_bytes(int32_t n_tensors, int32_t n_groups, int64_t n_chunks, uint64_t* step_bytes_host,
                                      uint64_t* groups_offset_host, uint64_t* chunk_bytes_host, uint64_t* partials_bytes_host) {
    if (n_tensors < 0 || n_groups < 0 || n_chunks < 0) return HGT_ERR_INVALID_ARG;
    if (!step_bytes_host || !groups_offset_host || !chunk_bytes_host || !partials_bytes_host) return HGT_ERR_INVALID_ARG;
    if (n_chunks > INT_MAX) return HGT_ERR_UNSUPPORTED;
    *groups_offset_host = (uint64_t)n_tensors * sizeof(hgt_optim_tensor);
    *step_bytes_host = *groups_offset_host + (uint64_t)n_groups * sizeof(hgt_optim_group);
    *chunk_bytes_host = (uint64_t)n_chunks * sizeof(hgt_optim_chunk);
    *partials_bytes_host = (uint64_t)n_chunks * sizeof(double);
    return HGT_OK;
}

extern "C" int hgt_grad_sqnorm(const hgt_optim_tensor* tensors, int32_t n_tensors, const hgt_optim_group* groups, int32_t n_groups,
                               const hgt_optim_chunk* chunks, int64_t n_chunks, double* partials, void* stream) {
    const int rc = optim_args_ok(tensors, n_tensors, groups, n_groups, chunks, n_chunks);
    if (rc != HGT_OK || n_chunks == 0) return rc;
    if (!partials) return HGT_ERR_INVALID_ARG;
    OptArgs A = {};
    A.tensors = tensors; A.groups = groups; A.chunks = chunks; A.partials = partials; A.n_tensors = n_tensors; A.n_groups = n_groups;
    k_grad_sqnorm<<<(unsigned)n_chunks, OPT_BLOCK, 0, (hipStream_t)stream>>>(A);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_grad_norm_join(const double* partials, int64_t n_chunks, float* total_norm, void* stream) {
    if (n_chunks < 0 || !total_norm || (n_chunks > 0 && !partials)) return HGT_ERR_INVALID_ARG;
    if (n_chunks > INT_MAX) return HGT_ERR_UNSUPPORTED;
    k_grad_norm_join<<<1, OPT_BLOCK, 0, (hipStream_t)stream>>>(partials, n_chunks, total_norm);      // no chunk: a norm of 0
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

extern "C" int hgt_adamw_step(const hgt_optim_tensor* tensors, int32_t n_tensors, const hgt_optim_group* groups, int32_t n_groups,
                              const hgt_optim_chunk* chunks, int64_t n_chunks, const float* total_norm, float max_norm, void* stream) {
    const int rc = optim_args_ok(tensors, n_tensors, groups, n_groups, chunks, n_chunks);
    if (rc != HGT_OK) return rc;
    if (total_norm && !(max_norm >= 0.0f)) return HGT_ERR_INVALID_ARG;             // negative or NaN
    if (n_chunks == 0) return HGT_OK;
    OptArgs A = {};
    A.tensors = tensors; A.groups = groups; A.chunks = chunks; A.total_norm = total_norm; A.max_norm = max_norm;
    A.n_tensors = n_tensors; A.n_groups = n_groups;
    k_adamw_step<<<(unsigned)n_chunks, OPT_BLOCK, 0, (hipStream_t)stream>>>(A);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}
