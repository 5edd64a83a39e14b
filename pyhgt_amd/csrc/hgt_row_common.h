// What the row kernels of hgt_task_loss.hip and hgt_task_vote.hip share: a wavefront (T = 64) or a workgroup (T = CL_BLOCK) per row of
// float32, position j of a row always in the same thread, partial results joined by a shuffle tree and then wavefront after wavefront.
// The float32 log-softmax parts (m, ls) of a row are formed here once, so that every kernel that needs logp_j = (x_j - m) - ls gets
// the same bits for it.
#ifndef HGT_ROW_COMMON_H_
#define HGT_ROW_COMMON_H_
#include <math.h>

#include "hgt_common.h"

namespace {

constexpr int CL_BLOCK = 256;
constexpr int CL_WAVES = CL_BLOCK / 64;
static_assert(HGT_CLASS_LOSS_WAVE_COLS == 4 * 64, "a wavefront row is one quad per lane");

// positions j .. j + 3 of a row (j a multiple of 4): one 16-byte load where the base is aligned and the four lie inside
__device__ __forceinline__ void load4(const float* p, int j, int C, bool vec, float fill, float (&v)[4]) {
    if (vec && j + 3 < C) {
        const float4 t = *reinterpret_cast<const float4*>(p + j);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = j + e < C ? p[j + e] : fill;
    }
}

// T threads (a wavefront or the workgroup) join their values: a shuffle tree, then the wavefronts in order; every thread gets the
// result.  S: the kernel's LDS scratch, with a member `float f[CL_WAVES]`
template <int T, class Scr>
__device__ __forceinline__ float group_max(float v, Scr& S) {
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if (T == 64) return v;
    if ((threadIdx.x & 63) == 0) S.f[threadIdx.x >> 6] = v;
    __syncthreads();
    v = S.f[0];
    for (int q = 1; q < CL_WAVES; ++q) v = fmaxf(v, S.f[q]);
    __syncthreads();
    return v;
}

template <int T, class Scr>
__device__ __forceinline__ float group_sum(float v, Scr& S) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if (T == 64) return v;
    if ((threadIdx.x & 63) == 0) S.f[threadIdx.x >> 6] = v;
    __syncthreads();
    v = S.f[0];
    for (int q = 1; q < CL_WAVES; ++q) v += S.f[q];
    __syncthreads();
    return v;
}

// m = max x and ls = log(sum exp(x - m)) of the row x[0 .. C), thread k of its T; a wavefront row (C <= 256) is read once and stays
// in `own` (positions 4 k .. 4 k + 3, -inf behind the end), a workgroup row is streamed twice
template <int T, class Scr>
__device__ __forceinline__ void row_lse(const float* x, int C, bool vec, int k, float (&own)[4], Scr& S, float& m, float& ls) {
    if (T == 64) load4(x, 4 * k, C, vec, -INFINITY, own);
    m = -INFINITY;
    if (T == 64) {
#pragma unroll
        for (int e = 0; e < 4; ++e) m = fmaxf(m, own[e]);
    } else {
        for (int j = 4 * k; j < C; j += 4 * T) {
            float v[4];
            load4(x, j, C, vec, -INFINITY, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) m = fmaxf(m, v[e]);
        }
    }
    m = group_max<T>(m, S);
    float sum = 0.0f;                                                             // (fmaxf drops a NaN logit, exp(NaN - m) keeps it)
    if (T == 64) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * k + e < C) sum += expf(own[e] - m);
        }
    } else {
        for (int j = 4 * k; j < C; j += 4 * T) {
            float v[4];
            load4(x, j, C, vec, -INFINITY, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (j + e < C) sum += expf(v[e] - m);
            }
        }
    }
    sum = group_sum<T>(sum, S);
    ls = logf(sum);
}

}  // namespace
#endif  // HGT_ROW_COMMON_H_
