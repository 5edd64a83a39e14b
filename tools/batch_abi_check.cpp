// Stand-alone host program for the argument checks of the batched sampler entry points (hgt_sampler_*_batched,
// hgt_sampler_gather_features): tables at the limits of the kernel-argument space (16 types, 48 triples), n_batch below 1, at and above
// HGT_SAMPLER_MAX_BATCH, NULL per-replica arrays, negative sizes, scratch one entry short of the requirement per replica.  Every call
// returns before a launch, so the program needs no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/batch_abi_check.cpp pyhgt_amd/csrc/hgt_sampler.hip -o batch_abi_check && ./batch_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "batch_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    const int T = HGT_SAMPLER_MAX_TYPES, M = HGT_SAMPLER_MAX_TRIPLES, R = M + 1, B = HGT_SAMPLER_MAX_BATCH;
    std::vector<uint64_t> buf(64, 0);      // host memory behind every pointer of the tables: no call may reach a kernel
    void* p = buf.data();
    std::vector<hgt_sampler_type> types(T);
    for (int t = 0; t < T; ++t)
        types[t] = hgt_sampler_type{(uint64_t*)p, (uint64_t*)p, (int32_t*)p, (int32_t*)p, (int32_t*)p, (int32_t*)p, 8, 4, 8, 0};
    std::vector<hgt_sampler_triple> triples(M);
    for (int m = 0; m < M; ++m) triples[m] = hgt_sampler_triple{(int32_t*)p, (int32_t*)p, (int32_t*)p, m % T, (m + 1) % T, m, 0};
    std::vector<hgt_sampler_mask> masks(M, hgt_sampler_mask{INT_MAX, INT_MAX});
    std::vector<uint64_t> seeds(B, ~0ull);      // exactly n_batch entries: a read past the end is the sanitizer's to find
    const hgt_sampler_type* ty = types.data();
    const hgt_sampler_triple* tr = triples.data();
    int32_t* q = (int32_t*)p;
    uint64_t* k = (uint64_t*)p;
    int64_t slots = 0;
    EXPECT(hgt_sampler_induce_slots(ty, T, tr, M, &slots), HGT_OK);
    if (slots != 4 * M) ++failures;
    const int into0 = M / T;      // triples into type 0: m % T == 0

    // n_batch: below 1, above the limit; at the limit the call goes on to the next check
    for (int nb : {0, -1, INT_MIN}) {
        EXPECT(hgt_sampler_seed_batched(ty, T, nb, 0, q, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, nb, 0, 0, 4, 2, 0, 0, seeds.data(), q, 64, nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_select_batched(ty, T, nb, 0, 0, 4, seeds.data(), k, q, 8, nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_induce_count_batched(ty, T, tr, M, nb, R, q, q, slots + 1, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, nb, R, q, q, slots + 1, q, q, q, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_reset_batched(ty, T, nb, nullptr), HGT_ERR_INVALID_ARG);
    }
    for (int nb : {B + 1, INT_MAX}) {
        EXPECT(hgt_sampler_seed_batched(ty, T, nb, 0, q, q, 2, 0, nullptr), HGT_ERR_UNSUPPORTED);
        EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, nb, 0, 0, 4, 2, 0, 0, seeds.data(), q, 64, nullptr), HGT_ERR_UNSUPPORTED);
        EXPECT(hgt_sampler_select_batched(ty, T, nb, 0, 0, 4, seeds.data(), k, q, 8, nullptr), HGT_ERR_UNSUPPORTED);
        EXPECT(hgt_sampler_induce_count_masked_batched(ty, T, tr, M, nb, R, q, q, slots + 1, q, q, q, masks.data(), nullptr), HGT_ERR_UNSUPPORTED);
        EXPECT(hgt_sampler_induce_fill_masked_batched(ty, T, tr, M, nb, R, q, q, slots + 1, q, q, q, 4, 6, q, q, q, q, q, masks.data(), nullptr),
               HGT_ERR_UNSUPPORTED);
        EXPECT(hgt_sampler_reset_batched(ty, T, nb, nullptr), HGT_ERR_UNSUPPORTED);
    }
    // seed: capacity, arrays, sizes (n_batch at its limit)
    EXPECT(hgt_sampler_seed_batched(ty, T, B, 0, q, q, 5, 0, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_seed_batched(ty, T, B, 0, nullptr, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed_batched(ty, T, B, 0, q, nullptr, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed_batched(ty, T, B, 0, q, q, -1, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed_batched(ty, T, B, T, q, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed_batched(nullptr, T, B, 0, q, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    // add_budget: all n_batch seeds are read, then the scratch is one entry short per replica
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, 4, 2, 0, 0, seeds.data(), q, 2 * into0, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, 4, 2, 0, 0, nullptr, q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, 4, 2, 0, 0, seeds.data(), nullptr, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, 4, -1, 0, 0, seeds.data(), q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, 2, 0, 0, seeds.data(), q, 64, nullptr),
           HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, 4, 0, 0, 0, seeds.data(), nullptr, 0, nullptr), HGT_OK);      // no row
    std::vector<uint64_t> one_seed(1, 7);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, 1, 0, 0, 4, 2, 0, 0, one_seed.data(), q, 2 * into0, nullptr), HGT_ERR_WORKSPACE);
    // select
    EXPECT(hgt_sampler_select_batched(ty, T, B, 0, 0, 4, seeds.data(), k, q, 7, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_select_batched(ty, T, B, 0, 0, 4, nullptr, k, q, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select_batched(ty, T, B, 0, 0, 4, seeds.data(), nullptr, q, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select_batched(ty, T, B, 0, 0, 4, seeds.data(), k, nullptr, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select_batched(ty, T, 1, 0, 0, 4, one_seed.data(), k, q, 7, nullptr), HGT_ERR_WORKSPACE);
    // induce: good masks pass on to the next check (the scratch is one entry short), bad ones stop the call
    EXPECT(hgt_sampler_induce_count_batched(ty, T, tr, M, B, R, q, q, slots, q, q, q, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_count_masked_batched(ty, T, tr, M, B, R, q, q, slots, q, q, q, masks.data(), nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_count_masked_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count_batched(ty, T, tr, M, B, R, nullptr, q, slots + 1, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots, q, q, q, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_fill_masked_batched(ty, T, tr, M, B, R, q, q, slots, q, q, q, 4, 6, q, q, q, q, q, masks.data(), nullptr),
           HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_fill_masked_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, q, 4, 6, q, q, q, q, q, nullptr, nullptr),
           HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, nullptr, q, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, nullptr, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, q, -1, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, q, 4, 3, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, q, 4, 6, nullptr, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, q, 4, 6, q, q, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, q, 4, (int64_t)INT_MAX + 1, q, q, q, q, q, nullptr),
           HGT_ERR_TOO_LARGE);
    for (int m : {0, M - 1}) {
        std::vector<hgt_sampler_mask> bad(M, hgt_sampler_mask{0, 0});
        (m ? bad[m].src_below : bad[m].tgt_below) = m ? INT_MIN : -1;
        EXPECT(hgt_sampler_induce_count_masked_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, q, bad.data(), nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_induce_fill_masked_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, q, q, 4, 6, q, q, q, q, q, bad.data(), nullptr),
               HGT_ERR_INVALID_ARG);
    }
    // reset
    EXPECT(hgt_sampler_reset_batched(nullptr, T, B, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_reset_batched(ty, T + 1, B, nullptr), HGT_ERR_UNSUPPORTED);

    // two checks fail at once: the code is that of the first -- the tables (and for the induce calls the relations), n_batch, the
    // seeds (the masks), then what the single entry point checks in its own order
    EXPECT(hgt_sampler_seed_batched(nullptr, T, B + 1, 0, q, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed_batched(ty, T + 1, 0, 0, q, q, 2, 0, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_seed_batched(ty, T, B + 1, T, q, q, 2, 0, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_seed_batched(ty, T, 0, 0, q, q, 5, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed_batched(ty, T, B, 0, nullptr, nullptr, 5, 0, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_add_budget_batched(nullptr, T, tr, M, B + 1, 0, 0, 4, 2, 0, 0, seeds.data(), q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B + 1, 0, 0, 4, 2, 0, 0, nullptr, q, 64, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, 2, 0, 0, nullptr, q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, T, 0, 4, 2, 0, 0, seeds.data(), q, 2 * into0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, -1, 0, 0, seeds.data(), q, 64, nullptr),
           HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, 2, 0, 0, seeds.data(), q, 2 * into0, nullptr),
           HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, 4, INT_MAX, 0, 0, seeds.data(), nullptr, 0, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, B, 0, 0, 4, 2, 0, 0, seeds.data(), nullptr, 2 * into0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget_batched(ty, T, tr, M, 0, 0, 0, 4, 0, 0, 0, seeds.data(), nullptr, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select_batched(ty, T + 1, 0, 0, 0, 4, seeds.data(), k, q, 8, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_select_batched(ty, T, B + 1, 0, 0, 4, nullptr, k, q, 8, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_select_batched(ty, T, B, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, nullptr, k, q, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select_batched(ty, T, B, T, 0, 4, seeds.data(), k, q, 7, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select_batched(ty, T, B, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, seeds.data(), nullptr, q, 7, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_select_batched(ty, T, B, 0, 0, 4, seeds.data(), nullptr, q, 7, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count_batched(ty, T, tr, M, B + 1, 0, q, q, slots + 1, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count_masked_batched(ty, T, tr, M, B + 1, R, q, q, slots + 1, q, q, q, nullptr, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_induce_count_masked_batched(ty, T, tr, M, B, R, nullptr, q, slots, q, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count_batched(ty, T, tr, M, 0, R, q, q, slots, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count_batched(ty, T, tr, M, B, R, nullptr, q, slots, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B + 1, 0, q, q, slots + 1, q, q, q, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_masked_batched(ty, T, tr, M, B + 1, R, q, q, slots + 1, q, q, q, 4, 6, q, q, q, q, q, nullptr, nullptr),
           HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots, q, q, q, 4, (int64_t)INT_MAX + 1, q, q, q, q, q, nullptr),
           HGT_ERR_TOO_LARGE);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots + 1, q, nullptr, q, 4, (int64_t)INT_MAX + 1, q, q, q, q, q, nullptr),
           HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_batched(ty, T, tr, M, B, R, q, q, slots, q, q, q, 4, 6, nullptr, q, q, q, q, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_reset_batched(ty, T + 1, 0, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_reset_batched(nullptr, T, B + 1, nullptr), HGT_ERR_INVALID_ARG);

    // features: exactly n_types pointers and row counts are read
    std::vector<const float*> feats(T, (const float*)p);
    std::vector<int32_t> rows(T, 8);
    float* out = (float*)p;
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B, 4, q, q, q, 0, out, nullptr), HGT_OK);      // no row: no launch
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B, 0, q, q, q, 3, out, nullptr), HGT_OK);      // no column
    EXPECT(hgt_sampler_gather_features(nullptr, rows.data(), T, B, 4, q, q, q, 3, out, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_gather_features(feats.data(), nullptr, T, B, 4, q, q, q, 3, out, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), 0, B, 4, q, q, q, 3, out, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T + 1, B, 4, q, q, q, 3, out, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, 0, 4, q, q, q, 3, out, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B + 1, 4, q, q, q, 3, out, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B, -1, q, q, q, 3, out, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B, 4, q, q, q, -1, out, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B, 4, nullptr, q, q, 3, out, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B, 4, q, nullptr, q, 3, out, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B, 4, q, q, nullptr, 3, out, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B, 4, q, q, q, 3, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    rows[T - 1] = -1;
    EXPECT(hgt_sampler_gather_features(feats.data(), rows.data(), T, B, 4, q, q, q, 3, out, nullptr), HGT_ERR_INVALID_ARG);

    return abi_check_report("batch_abi_check");
}
