// Stand-alone host program for the argument checks of the single sampler entry points (hgt_sampler_seed, _add_budget, _select,
// _induce_slots, _induce_count[_masked], _induce_fill[_masked], _reset): the cases of batch_abi_check.cpp without n_batch.  Tables at the
// limits of the kernel-argument space (16 types, 48 triples), NULL arrays, negative sizes, scratch one entry short, sizes past the
// limits, bad and missing masks, the HGT_OK returns without work, and calls in which two checks fail at once: the code named is the one
// of the check that comes first, so the order of the checks is part of what is pinned.  Every call returns before a launch, so the
// program needs no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/sampler_abi_check.cpp pyhgt_amd/csrc/hgt_sampler.hip -o sampler_abi_check && ./sampler_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "sampler_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    const int T = HGT_SAMPLER_MAX_TYPES, M = HGT_SAMPLER_MAX_TRIPLES, R = M + 1;
    std::vector<uint64_t> buf(64, 0);      // host memory behind every pointer of the tables: no call may reach a kernel
    void* p = buf.data();
    std::vector<hgt_sampler_type> types(T);
    for (int t = 0; t < T; ++t)
        types[t] = hgt_sampler_type{(uint64_t*)p, (uint64_t*)p, (int32_t*)p, (int32_t*)p, (int32_t*)p, (int32_t*)p, 8, 4, 8, 0};
    std::vector<hgt_sampler_triple> triples(M);
    for (int m = 0; m < M; ++m) triples[m] = hgt_sampler_triple{(int32_t*)p, (int32_t*)p, (int32_t*)p, m % T, (m + 1) % T, m, 0};
    std::vector<hgt_sampler_mask> masks(M, hgt_sampler_mask{INT_MAX, INT_MAX});
    const hgt_sampler_type* ty = types.data();
    const hgt_sampler_triple* tr = triples.data();
    const hgt_sampler_mask* mk = masks.data();
    int32_t* q = (int32_t*)p;
    uint64_t* k = (uint64_t*)p;
    const uint64_t seed = ~0ull;
    const int into0 = M / T;      // triples into type 0: m % T == 0
    const int64_t big = (int64_t)INT_MAX + 1;

    // induce_slots: host only
    int64_t slots = 0;
    EXPECT(hgt_sampler_induce_slots(ty, T, tr, M, &slots), HGT_OK);
    CHECK(slots == 4 * M);
    EXPECT(hgt_sampler_induce_slots(ty, T, tr, M, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_slots(nullptr, T, tr, M, &slots), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_slots(ty, T, nullptr, M, &slots), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_slots(ty, 0, tr, M, &slots), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_slots(ty, T, tr, -1, &slots), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_slots(ty, T + 1, tr, M, &slots), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_induce_slots(ty, T, tr, M + 1, &slots), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_induce_slots(ty, T + 1, tr, M, nullptr), HGT_ERR_INVALID_ARG);      // the out pointer comes before the tables
    slots = 4 * M;

    // seed: capacity, arrays, sizes
    EXPECT(hgt_sampler_seed(ty, T, 0, q, q, 5, 0, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_seed(ty, T, 0, nullptr, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed(ty, T, 0, q, nullptr, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed(ty, T, 0, q, q, -1, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed(ty, T, 0, q, q, 2, -1, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed(ty, T, T, q, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed(ty, T, -1, q, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed(nullptr, T, 0, q, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed(ty, T + 1, 0, q, q, 2, 0, nullptr), HGT_ERR_UNSUPPORTED);
    // two at once: the tables, then type / n / step, then the capacity, then the arrays
    EXPECT(hgt_sampler_seed(ty, T + 1, T + 1, q, q, 2, 0, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_seed(nullptr, T + 1, 0, q, q, 2, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed(ty, T, 0, q, q, 5, -1, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_seed(ty, T, 0, nullptr, nullptr, 5, 0, nullptr), HGT_ERR_WORKSPACE);

    // add_budget: rows = max_new x triples into the type; the scratch is one entry short
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, 4, 2, 0, 0, seed, q, 2 * into0, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, 4, 2, 0, 0, seed, nullptr, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, 4, -1, 0, 0, seed, q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, -1, 4, 2, 0, 0, seed, q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, T, 0, 4, 2, 0, 0, seed, q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, 0, 2, 0, 0, seed, q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, 2, 0, 0, seed, q, 64, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, 4, INT_MAX, 0, 0, seed, q, 64, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_sampler_add_budget(nullptr, T, tr, M, 0, 0, 4, 2, 0, 0, seed, q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget(ty, T, nullptr, M, 0, 0, 4, 2, 0, 0, seed, q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M + 1, 0, 0, 4, 2, 0, 0, seed, q, 64, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, 4, 0, 0, 0, seed, nullptr, 0, nullptr), HGT_OK);      // no row
    EXPECT(hgt_sampler_add_budget(ty, T, nullptr, 0, 0, 0, 4, 2, 0, 0, seed, nullptr, 0, nullptr), HGT_OK);  // no triple into the type
    {
        std::vector<hgt_sampler_triple> bad(triples);      // a triple into type 0 without its time array
        bad[T].time = nullptr;
        EXPECT(hgt_sampler_add_budget(ty, T, bad.data(), M, 0, 0, 4, 2, 0, 0, seed, q, 64, nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_add_budget(ty, T, bad.data(), M, 0, 0, 4, 0, 0, 0, seed, nullptr, 0, nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_add_budget(ty, T, bad.data(), M, 1, 0, 4, 2, 0, 0, seed, q, 2 * into0, nullptr), HGT_ERR_WORKSPACE);
    }
    // two at once: tables, then type / step / sizes, then the sampled_number limit, then rows, hub, scratch
    EXPECT(hgt_sampler_add_budget(ty, T + 1, tr, M, T + 1, 0, 4, 2, 0, 0, seed, q, 64, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, T, 0, 4, 2, 0, 0, seed, q, 2 * into0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, -1, 0, 0, seed, q, 64, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, 2, 0, 0, seed, q, 2 * into0, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, 0, 0, 0, seed, nullptr, 0, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, 4, INT_MAX, 0, 0, seed, nullptr, 0, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_sampler_add_budget(ty, T, tr, M, 0, 0, 4, 2, 0, 0, seed, nullptr, 2 * into0, nullptr), HGT_ERR_INVALID_ARG);

    // select
    EXPECT(hgt_sampler_select(ty, T, 0, 0, 4, seed, k, q, 7, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_select(ty, T, 0, 0, 4, seed, nullptr, q, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select(ty, T, 0, 0, 4, seed, k, nullptr, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select(ty, T, T, 0, 4, seed, k, q, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select(ty, T, 0, -1, 4, seed, k, q, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select(ty, T, 0, 0, 0, seed, k, q, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select(ty, T, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, seed, k, q, 8, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_select(nullptr, T, 0, 0, 4, seed, k, q, 8, nullptr), HGT_ERR_INVALID_ARG);
    {
        std::vector<hgt_sampler_type> none(types);      // a type that can have no candidate: nothing to do, whatever the scratch is
        none[0].cap_cand = 0;
        none[0].cand = nullptr;
        EXPECT(hgt_sampler_select(none.data(), T, 0, 0, 4, seed, nullptr, nullptr, 0, nullptr), HGT_OK);
        EXPECT(hgt_sampler_select(none.data(), T, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, seed, nullptr, nullptr, 0, nullptr), HGT_ERR_UNSUPPORTED);
        EXPECT(hgt_sampler_select(none.data(), T, 1, 0, 4, seed, k, q, 7, nullptr), HGT_ERR_WORKSPACE);
    }
    // two at once: tables, type / step / sampled_number, its limit, the arrays, the scratch
    EXPECT(hgt_sampler_select(ty, T + 1, T + 1, 0, 4, seed, k, q, 8, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_select(ty, T, T, 0, 4, seed, k, q, 7, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select(ty, T, -1, 0, HGT_SAMPLER_MAX_NUMBER + 1, seed, k, q, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_select(ty, T, 0, 0, HGT_SAMPLER_MAX_NUMBER + 1, seed, nullptr, q, 7, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_select(ty, T, 0, 0, 4, seed, nullptr, q, 7, nullptr), HGT_ERR_INVALID_ARG);

    // induce: good masks pass on to the next check (the scratch is one entry short), bad ones stop the call
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R, q, q, slots, q, q, q, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_count_masked(ty, T, tr, M, R, q, q, slots, q, q, q, mk, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_count_masked(ty, T, tr, M, R, q, q, slots + 1, q, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R, nullptr, q, slots + 1, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R, q, nullptr, slots + 1, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R, q, q, slots + 1, nullptr, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R, q, q, slots + 1, q, nullptr, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R, q, q, slots + 1, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R, q, q, -1, q, q, q, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, 0, q, q, slots + 1, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R + 1, q, q, slots + 1, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R - 1, q, q, slots + 1, q, q, q, nullptr), HGT_ERR_INVALID_ARG);      // rel_id M - 1 is `self`
    EXPECT(hgt_sampler_induce_count(nullptr, T, tr, M, R, q, q, slots + 1, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T + 1, tr, M, R, q, q, slots + 1, q, q, q, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots, q, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_fill_masked(ty, T, tr, M, R, q, q, slots, q, 4, 6, q, q, q, q, q, mk, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_fill_masked(ty, T, tr, M, R, q, q, slots + 1, q, 4, 6, q, q, q, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, nullptr, q, slots + 1, q, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, nullptr, slots + 1, q, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, nullptr, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, -1, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, 4, 3, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, 4, 6, nullptr, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, 4, 6, q, nullptr, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, 4, 6, q, q, nullptr, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, 4, 6, q, q, q, nullptr, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, 4, 6, q, q, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, 4, big, q, q, q, q, q, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, 0, q, q, slots + 1, q, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_sampler_induce_fill_masked(ty, T, tr, M, R, q, q, slots + 1, q, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, mk, nullptr),
           HGT_OK);
    for (int m : {0, M - 1}) {
        std::vector<hgt_sampler_mask> bad(M, hgt_sampler_mask{0, 0});
        (m ? bad[m].src_below : bad[m].tgt_below) = m ? INT_MIN : -1;
        EXPECT(hgt_sampler_induce_count_masked(ty, T, tr, M, R, q, q, slots + 1, q, q, q, bad.data(), nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_induce_fill_masked(ty, T, tr, M, R, q, q, slots + 1, q, 4, 6, q, q, q, q, q, bad.data(), nullptr),
               HGT_ERR_INVALID_ARG);
        // two at once: the masks come before the scratch and before the size of the result
        EXPECT(hgt_sampler_induce_count_masked(ty, T, tr, M, R, q, q, slots, q, q, q, bad.data(), nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_induce_fill_masked(ty, T, tr, M, R, q, q, slots, q, 4, big, q, q, q, q, q, bad.data(), nullptr), HGT_ERR_INVALID_ARG);
    }
    // two at once: tables and relations, the masks, the arrays and sizes, n_edges, the scratch, the outputs
    EXPECT(hgt_sampler_induce_count_masked(ty, T + 1, tr, M, R, q, q, slots + 1, q, q, q, nullptr, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, 0, q, q, slots, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count(ty, T, tr, M, R, nullptr, q, slots, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count_masked(ty, T, tr, M, R, nullptr, q, slots, q, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_masked(ty, T + 1, tr, M, R, q, q, slots + 1, q, 4, 6, q, q, q, q, q, nullptr, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots, q, 4, big, q, q, q, q, q, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, nullptr, q, slots + 1, q, 4, big, q, q, q, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots, q, 4, 6, nullptr, q, q, q, q, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_fill(ty, T, tr, M, R, q, q, slots + 1, q, 4, big, nullptr, q, q, q, q, nullptr), HGT_ERR_TOO_LARGE);

    // reset
    EXPECT(hgt_sampler_reset(nullptr, T, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_reset(ty, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_reset(ty, T + 1, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_reset(nullptr, T + 1, nullptr), HGT_ERR_INVALID_ARG);
    {
        std::vector<hgt_sampler_type> bad(types);      // a table entry without its counters
        bad[T - 1].counts = nullptr;
        EXPECT(hgt_sampler_reset(bad.data(), T, nullptr), HGT_ERR_INVALID_ARG);
        EXPECT(hgt_sampler_seed(bad.data(), T, 0, q, q, 5, 0, nullptr), HGT_ERR_INVALID_ARG);
    }

    return abi_check_report("sampler_abi_check");
}
