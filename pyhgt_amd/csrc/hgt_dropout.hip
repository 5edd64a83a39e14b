// Counter-based dropout (gfx950): a mask that is a pure function of (seed, offset, keep, element index), so the training step's
// recompute mode (pyhgt_amd/autograd.py, recompute=True) keeps a seed instead of an [NQ, out_dim] float mask per dropout site
// (conv.py:125 / 261,273) and the backward writes the mask again when it needs it.
//
//   generator  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
//   key        (seed & 0xffffffff, seed >> 32)
//   counter    the 64-bit value offset + i / 4 in words 0 and 1 (carry into word 1), words 2 and 3 zero
//   element i  takes output word i % 4 and is kept iff word < (uint32)(keep * 2^32)
//   mask       1.0f / keep where kept, 0 elsewhere;  apply: x[i] *= that float (bit-identical to hgt_mul_inplace(x, mask))
//   keep >= 1  every element kept, factor 1;  keep <= 0: zeros (the Dropout(p=1) rule of hgt_conv_train)
//
// One Philox call serves four consecutive floats: a lane owns the group [4q, 4q + 4) -- one 16-byte load and one 16-byte store
// (mask: the store alone).  A pointer that is not 16-byte aligned and the last n % 4 elements go element by element, still one
// Philox call per group.  Each of the ten rounds is two 32 x 32 -> 64-bit products (v_mad_u64_u32 gives high and low half at once),
// three XORs and two key additions: ~70 integer instructions per 16 bytes against 2 (apply) / 1 (mask) memory instructions.
// Whether that leaves the kernel HBM-bound has not been measured here; tools/bench_train.py times it against hgt_mul_inplace.
#include "hgt_common.h"
#include "hgt_philox.h"      // philox4x32_10(counter, k0, k1), shared with hgt_sampler.hip

namespace {

// APPLY: x[i] *= factor_i, else x[i] = factor_i.  Grid-stride over the groups of four elements; n_groups = ceil(n / 4).
// keep_all: keep >= 1 (every word passes; thr cannot hold 2^32).  vec_ok: x is 16-byte aligned.
template <bool APPLY>
__global__ void __launch_bounds__(256) k_dropout(float* __restrict__ x, int64_t n, int64_t n_groups, uint64_t offset, uint32_t k0, uint32_t k1,
                                                 uint32_t thr, int keep_all, float inv_keep, int vec_ok) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_groups; q += stride) {
        const Philox4 r = philox4x32_10(offset + (uint64_t)q, k0, k1);
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = (keep_all || r.w[j] < thr) ? inv_keep : 0.0f;
        const int64_t i0 = 4 * q;
        if (vec_ok && i0 + 4 <= n) {
            float4* p = reinterpret_cast<float4*>(x + i0);
            float4 v;
            if constexpr (APPLY) {
                v = *p;
                v.x *= f[0]; v.y *= f[1]; v.z *= f[2]; v.w *= f[3];
            } else {
                v = make_float4(f[0], f[1], f[2], f[3]);
            }
            *p = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j < n) {
                    if constexpr (APPLY) x[i0 + j] *= f[j];
                    else x[i0 + j] = f[j];
                }
            }
        }
    }
}

constexpr int64_t DROPOUT_MAX_BLOCKS = 8192;      // 256 CUs x 8 workgroups of 256 x 4: larger arrays take several passes of the grid

template <bool APPLY>
int dropout_launch(float* x, int64_t n, uint64_t seed, uint64_t offset, float keep, void* stream) {
    if (!x || n < 0 || keep != keep) return HGT_ERR_INVALID_ARG;
    if (n == 0) return HGT_OK;                    // before any runtime call
    const int keep_all = keep >= 1.0f;
    const bool none = keep <= 0.0f;
    // keep in (0, 1): keep * 2^32 is exact in double and below 2^32
    const uint32_t thr = (keep_all || none) ? 0u : (uint32_t)((double)keep * 4294967296.0);
    const float inv_keep = keep_all ? 1.0f : (none ? 0.0f : 1.0f / keep);
    const int64_t n_groups = (n + 3) / 4;
    const int64_t blocks = (n_groups + 255) / 256;
    const unsigned grid = (unsigned)(blocks < DROPOUT_MAX_BLOCKS ? blocks : DROPOUT_MAX_BLOCKS);
    const int vec_ok = ((uintptr_t)x & 15) == 0;
    k_dropout<APPLY><<<grid, 256, 0, (hipStream_t)stream>>>(x, n, n_groups, offset, (uint32_t)seed, (uint32_t)(seed >> 32), thr, keep_all,
                                                            inv_keep, vec_ok);
    HGT_CHECK_LAUNCH();
    return HGT_OK;
}

}  // namespace

extern "C" int hgt_dropout_mask(float* m, int64_t n, uint64_t seed, uint64_t offset, float keep, void* stream) {
    return dropout_launch<false>(m, n, seed, offset, keep, stream);
}

extern "C" int hgt_dropout_apply(float* x, int64_t n, uint64_t seed, uint64_t offset, float keep, void* stream) {
    return dropout_launch<true>(x, n, seed, offset, keep, stream);
}
