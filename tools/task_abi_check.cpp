// Stand-alone host program for the argument checks of the task-batch entry points (hgt_sampler_induce_count_masked,
// hgt_sampler_induce_fill_masked, hgt_sampler_labels): tables at the limits of the kernel-argument space (16 types, 48 triples), masks
// at INT32_MAX, a negative threshold in the first and in the last entry, NULL tables and arrays.  Every call returns before a launch,
// so the program needs no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/task_abi_check.cpp pyhgt_amd/csrc/hgt_sampler.hip pyhgt_amd/csrc/hgt_sampler_labels.hip \
//         -o task_abi_check && ./task_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "task_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
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
    int32_t* q = (int32_t*)p;
    int64_t slots = 0;
    EXPECT(hgt_sampler_induce_slots(types.data(), T, triples.data(), M, &slots), HGT_OK);
    if (slots != 4 * M) ++failures;

    // masked induction: good masks pass on to the next check (the scratch is one entry short), bad ones stop the call
    EXPECT(hgt_sampler_induce_count_masked(types.data(), T, triples.data(), M, R, q, q, slots, q, q, q, masks.data(), nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_fill_masked(types.data(), T, triples.data(), M, R, q, q, slots, q, 4, 6, q, q, q, q, q, masks.data(), nullptr),
           HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_count_masked(types.data(), T, triples.data(), M, R, q, q, slots + 1, q, q, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_fill_masked(types.data(), T, triples.data(), M, R, q, q, slots + 1, q, 4, 6, q, q, q, q, q, nullptr, nullptr),
           HGT_ERR_INVALID_ARG);
    for (int m : {0, M - 1}) {
        for (int which = 0; which < 2; ++which) {
            std::vector<hgt_sampler_mask> bad(M, hgt_sampler_mask{0, 0});
            (which ? bad[m].src_below : bad[m].tgt_below) = m ? INT_MIN : -1;
            EXPECT(hgt_sampler_induce_count_masked(types.data(), T, triples.data(), M, R, q, q, slots + 1, q, q, q, bad.data(), nullptr),
                   HGT_ERR_INVALID_ARG);
            EXPECT(hgt_sampler_induce_fill_masked(types.data(), T, triples.data(), M, R, q, q, slots + 1, q, 4, 6, q, q, q, q, q, bad.data(),
                                                  nullptr),
                   HGT_ERR_INVALID_ARG);
        }
    }
    // more triples than the tables hold: the masks are not read
    EXPECT(hgt_sampler_induce_count_masked(types.data(), T, triples.data(), M + 1, R, q, q, slots + 1, q, q, q, masks.data(), nullptr),
           HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_sampler_induce_count_masked(types.data(), T, triples.data(), -1, R, q, q, slots + 1, q, q, q, masks.data(), nullptr),
           HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_induce_count_masked(nullptr, T, triples.data(), M, R, q, q, slots + 1, q, q, q, masks.data(), nullptr), HGT_ERR_INVALID_ARG);
    // a one-entry mask array with one triple: exactly that entry is read
    std::vector<hgt_sampler_mask> one(1, hgt_sampler_mask{0, -5});
    EXPECT(hgt_sampler_induce_count_masked(types.data(), T, triples.data(), 1, 2, q, q, 5, q, q, q, one.data(), nullptr), HGT_ERR_INVALID_ARG);
    one[0].src_below = 5;
    EXPECT(hgt_sampler_induce_count_masked(types.data(), T, triples.data(), 1, 2, q, q, 4, q, q, q, one.data(), nullptr), HGT_ERR_WORKSPACE);
    // the unmasked entry points take no masks and keep their rules
    EXPECT(hgt_sampler_induce_count(types.data(), T, triples.data(), M, R, q, q, slots, q, q, q, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_sampler_induce_fill(types.data(), T, triples.data(), M, R, q, q, slots, q, 4, 6, q, q, q, q, q, nullptr), HGT_ERR_WORKSPACE);

    // labels
    const hgt_sampler_triple* tr = &triples[0];
    float* d = (float*)p;
    EXPECT(hgt_sampler_labels(tr, 8, 8, q, 0, q, 4, 0, 0, 0, d, 4, q, q, nullptr), HGT_OK);
    EXPECT(hgt_sampler_labels(nullptr, 0, 0, nullptr, 0, nullptr, 0, 0, 0, 0, nullptr, 0, nullptr, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_sampler_labels(nullptr, 8, 8, q, 2, q, 4, 0, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, 8, 8, nullptr, 2, q, 4, 0, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, 8, 8, q, 2, nullptr, 4, 0, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, 8, 8, q, INT_MIN, q, 4, 0, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, INT_MIN, 8, q, 2, q, 4, 0, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, 8, -1, q, 2, q, 4, 0, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, 8, 8, q, 2, q, -1, 0, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, 8, 8, q, 2, q, INT_MAX, 0, 0, 0, d, (int64_t)INT_MAX - 1, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, 8, 8, q, 2, q, 4, 0, 0, 0, d, -4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, 8, 8, q, 2, q, 4, 1, INT_MAX, INT_MIN, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(tr, 8, 8, q, 2, q, 4, 1, 1, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    hgt_sampler_triple no_src = *tr, no_time = *tr, no_indptr = *tr;
    no_src.src = nullptr;
    no_time.time = nullptr;
    no_indptr.indptr = nullptr;
    EXPECT(hgt_sampler_labels(&no_src, 8, 8, q, 2, q, 4, 0, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(&no_time, 8, 8, q, 2, q, 4, 1, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_labels(&no_indptr, 8, 8, q, 2, q, 4, 0, 0, 0, d, 4, q, q, nullptr), HGT_ERR_INVALID_ARG);

    return abi_check_report("task_abi_check");
}
