// Stand-alone host program for the argument checks of the classification-loss entry points (hgt_class_loss, hgt_class_loss_bwd,
// hgt_sampler_label_columns): no label form or several, sizes at the ends of their ranges, NULL arrays, leading dimensions below the
// row length, a list width below 1.  Every call returns before a launch, so the program needs no GPU; it is meant to be built with the
// host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/class_loss_abi_check.cpp pyhgt_amd/csrc/hgt_task_loss.hip pyhgt_amd/csrc/hgt_sampler_labels.hip \
//         -o class_loss_abi_check && ./class_loss_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "class_loss_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    std::vector<uint64_t> buf(64, 0);      // host memory behind every pointer: no call may reach a kernel
    float* f = (float*)buf.data();
    int32_t* i = (int32_t*)buf.data();
    const int64_t* q = (const int64_t*)buf.data();
    const float* nf = nullptr;
    const int64_t* nq = nullptr;
    const int32_t* ni = nullptr;

    // forward: nothing to do
    EXPECT(hgt_class_loss(nullptr, 0, 0, 0, nf, 0, q, ni, 0, ni, nullptr, nullptr, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_class_loss(f, 8, 0, 8, f, 8, nq, ni, 0, ni, f, f, f, nullptr), HGT_OK);
    EXPECT(hgt_class_loss(nullptr, -5, 0, INT_MAX, nf, -5, nq, i, 1, i, nullptr, nullptr, nullptr, nullptr), HGT_OK);
    // no label form, or more than one, even without a row
    EXPECT(hgt_class_loss(f, 8, 2, 8, nf, 0, nq, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 0, 8, nf, 0, nq, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, f, 8, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, f, 8, nq, i, 4, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, nf, 0, q, i, 4, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 0, 8, f, 8, q, i, 4, i, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, nf, 0, q, ni, 0, i, f, f, f, nullptr), HGT_ERR_INVALID_ARG);        // count without columns
    // negative sizes
    EXPECT(hgt_class_loss(f, 8, -1, 8, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, INT_MIN, 8, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, -1, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, INT_MIN, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, nf, 0, q, ni, -1, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    // a list narrower than one entry
    EXPECT(hgt_class_loss(f, 8, 2, 8, nf, 0, nq, i, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, nf, 0, nq, i, -3, i, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 0, 8, nf, 0, nq, i, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    // leading dimensions below the row length
    EXPECT(hgt_class_loss(f, 7, 2, 8, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, -8, 2, 8, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, LLONG_MIN, 2, 8, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, f, 7, nq, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, f, LLONG_MIN, nq, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    // NULL arrays with rows
    EXPECT(hgt_class_loss(nullptr, 8, 2, 8, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, nf, 0, q, ni, 0, ni, nullptr, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, nf, 0, q, ni, 0, ni, f, nullptr, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, 2, 8, nf, 0, q, ni, 0, ni, f, f, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss(f, 8, INT_MAX, 8, nf, 0, nq, i, INT_MAX, i, nullptr, f, f, nullptr), HGT_ERR_INVALID_ARG);
    // rows too long for 32-bit positions with a step past the end
    EXPECT(hgt_class_loss(f, LLONG_MAX, 2, INT_MAX, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_class_loss(f, LLONG_MAX, 2, INT_MAX - 1023, f, LLONG_MAX, nq, ni, 0, ni, f, f, f, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_class_loss(f, INT_MAX - 1025, 2, INT_MAX - 1024, nf, 0, q, ni, 0, ni, f, f, f, nullptr), HGT_ERR_INVALID_ARG);

    // backward: the same checks, then its own arrays
    EXPECT(hgt_class_loss_bwd(nullptr, 0, 0, 0, nf, 0, q, ni, 0, ni, nullptr, nullptr, nullptr, nullptr, 0, nullptr), HGT_OK);
    EXPECT(hgt_class_loss_bwd(f, 8, 0, 8, nf, 0, nq, i, 4, i, f, f, f, f, -1, nullptr), HGT_OK);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, nf, 0, nq, ni, 0, ni, f, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, f, 8, q, ni, 0, ni, f, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, f, 8, q, i, 4, i, f, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, -1, 8, nf, 0, q, ni, 0, ni, f, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, -1, nf, 0, q, ni, 0, ni, f, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, nf, 0, nq, i, 0, ni, f, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 7, 2, 8, nf, 0, q, ni, 0, ni, f, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, f, 7, nq, ni, 0, ni, f, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, nf, 0, q, ni, 0, ni, f, f, f, f, 7, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, nf, 0, q, ni, 0, ni, f, f, f, f, LLONG_MIN, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(nullptr, 8, 2, 8, nf, 0, q, ni, 0, ni, f, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, nf, 0, q, ni, 0, ni, nullptr, f, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, nf, 0, q, ni, 0, ni, f, nullptr, f, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, 2, 8, nf, 0, q, ni, 0, ni, f, f, nullptr, f, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, 8, INT_MAX, 8, nf, 0, q, ni, 0, ni, f, f, f, nullptr, 8, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_loss_bwd(f, LLONG_MAX, 2, INT_MAX, nf, 0, q, ni, 0, ni, f, f, f, f, LLONG_MAX, nullptr), HGT_ERR_UNSUPPORTED);

    // the labels as column lists
    hgt_sampler_triple tr = {};
    tr.indptr = i, tr.src = i, tr.time = i;
    hgt_sampler_triple no_table = {};
    EXPECT(hgt_sampler_label_columns(nullptr, 0, 0, nullptr, 0, nullptr, 0, 0, 0, 0, nullptr, 1, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 0, i, INT_MAX, 1, -5, 5, nullptr, INT_MAX, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, -1, i, 8, 0, 0, 0, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&tr, -1, 4, i, 2, i, 8, 0, 0, 0, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&tr, 4, INT_MIN, i, 2, i, 8, 0, 0, 0, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 2, i, -1, 0, 0, 0, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 2, i, 8, 1, 6, 5, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);       // an empty window
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 2, i, 8, 0, 0, 0, i, 0, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 0, i, 8, 0, 0, 0, i, 0, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 2, i, 8, 0, 0, 0, i, INT_MIN, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 2, i, 8, 0, 0, 0, nullptr, 4, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(nullptr, 4, 4, i, 2, i, 8, 0, 0, 0, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&no_table, 4, 4, i, 2, i, 8, 0, 0, 0, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, nullptr, 2, i, 8, 0, 0, 0, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 2, nullptr, 8, 0, 0, 0, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);
    tr.time = nullptr;
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 2, i, 8, 1, 0, 5, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);       // a window without times
    tr.time = i, tr.src = nullptr;
    EXPECT(hgt_sampler_label_columns(&tr, 4, 4, i, 2, i, 8, 0, 0, 0, i, 4, i, nullptr), HGT_ERR_INVALID_ARG);

    return abi_check_report("class_loss_abi_check");
}
