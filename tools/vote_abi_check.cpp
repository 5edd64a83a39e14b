// Stand-alone host program for the argument checks of the voted-evaluation entry points (hgt_class_predict, hgt_vote_add): NULL
// arrays, outputs and labels that do not go together, sizes at the ends of their ranges, leading dimensions below the row length,
// split counts out of range, piece offsets that decrease, and every call that has nothing to do.  Every call returns before a launch
// or a runtime call, so the program needs no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/vote_abi_check.cpp pyhgt_amd/csrc/hgt_task_vote.hip -o vote_abi_check && ./vote_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "vote_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.  (n_rows == 0
// with counts_out zeroes the counts on the stream: that path needs a device and is covered by the GPU tests.)
#include <climits>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    std::vector<uint64_t> buf(64, 0);      // host memory behind every pointer: no call may reach a kernel
    float* f = (float*)buf.data();
    int32_t* i = (int32_t*)buf.data();
    int64_t* q = (int64_t*)buf.data();
    const int64_t* nq = nullptr;
    const int32_t* ni = nullptr;
    const int MAXS = HGT_PREDICT_MAX_SPLITS;

    // hgt_class_predict: nothing to do
    EXPECT(hgt_class_predict(nullptr, 0, 0, 0, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_class_predict(f, 8, 0, 8, q, 4, q, i, MAXS, q, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_class_predict(nullptr, INT_MAX, 0, INT_MAX, nq, 0, q, ni, 1, q, nullptr, nullptr), HGT_OK);
    // no output at all; counts or split without labels
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, q, ni, 1, nullptr, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 0, 8, nq, 0, q, ni, 1, nullptr, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, nq, ni, 1, q, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, nq, ni, 1, nullptr, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, nq, i, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, q, 4, nq, i, 3, q, i, nullptr), HGT_ERR_INVALID_ARG);
    // the number of splits
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, q, i, 0, q, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, q, i, -1, q, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, q, i, MAXS + 1, q, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, q, i, INT_MAX, q, i, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, q, ni, 2, q, i, nullptr), HGT_ERR_INVALID_ARG);            // without split: 1
    EXPECT(hgt_class_predict(f, 8, 2, 8, nq, 0, q, ni, 0, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 0, 8, nq, 0, q, i, MAXS + 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    // negative sizes
    EXPECT(hgt_class_predict(f, 8, -1, 8, nq, 0, q, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, INT_MIN, 8, nq, 0, q, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, -1, nq, 0, q, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, INT_MIN, nq, 0, q, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, q, -1, q, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 8, 2, 8, q, LLONG_MIN, q, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    // rows without a column, a leading dimension below the row length, NULL scores
    EXPECT(hgt_class_predict(f, 8, 2, 0, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 7, 2, 8, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, -8, 2, 8, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, LLONG_MIN, 2, 8, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(f, 7, 0, 8, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(nullptr, 8, 2, 8, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_class_predict(nullptr, 8, INT_MAX, 8, q, LLONG_MAX, q, i, MAXS, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    // rows too long for 32-bit positions with a step past the end
    EXPECT(hgt_class_predict(f, LLONG_MAX, 2, INT_MAX, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_class_predict(f, LLONG_MAX, 2, INT_MAX - 1023, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_class_predict(f, INT_MAX - 1025, 2, INT_MAX - 1024, nq, 0, nq, ni, 1, q, nullptr, nullptr), HGT_ERR_INVALID_ARG);

    // hgt_vote_add: nothing to do
    const int32_t none[4] = {0, 0, 0, 0}, late[3] = {5, 5, 5}, two[3] = {0, 2, 3}, back[3] = {0, 2, 1}, minus[2] = {-1, 2};
    EXPECT(hgt_vote_add(nullptr, 0, 0, nq, ni, 0, ni, 0, nullptr, 0, nullptr, 0, nullptr), HGT_OK);
    EXPECT(hgt_vote_add(f, 8, 8, q, ni, 0, i, 4, f, 8, i, 4, nullptr), HGT_OK);
    EXPECT(hgt_vote_add(nullptr, 8, 8, nq, none, 3, ni, 4, nullptr, 8, nullptr, 4, nullptr), HGT_OK);
    EXPECT(hgt_vote_add(nullptr, 0, 0, nq, late, 2, ni, 0, nullptr, 0, nullptr, 0, nullptr), HGT_OK);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, 0, f, 8, i, 4, nullptr), HGT_OK);                            // no node, no slot:
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, 4, f, 8, i, 0, nullptr), HGT_OK);                            // every row is skipped
    // the pieces
    EXPECT(hgt_vote_add(f, 8, 8, q, two, -1, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, INT_MIN, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, ni, 2, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, back, 2, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, minus, 1, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    // negative sizes
    EXPECT(hgt_vote_add(f, 8, -1, q, two, 2, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, INT_MIN, q, two, 2, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, -1, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, LLONG_MIN, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, 4, f, 8, i, -1, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, none, 3, i, 4, f, 8, i, INT_MIN, nullptr), HGT_ERR_INVALID_ARG);
    // leading dimensions below the row length; rows without a column
    EXPECT(hgt_vote_add(f, 7, 8, q, two, 2, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, LLONG_MIN, 8, q, two, 2, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, 4, f, 7, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, 4, f, -8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, none, 3, i, 4, f, 7, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 0, q, two, 2, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    // NULL arrays with rows
    EXPECT(hgt_vote_add(nullptr, 8, 8, q, two, 2, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, nq, two, 2, i, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, ni, 4, f, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, 4, nullptr, 8, i, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, 4, f, 8, nullptr, 4, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_vote_add(f, 8, 8, q, two, 2, i, 0, f, 8, nullptr, 0, nullptr), HGT_ERR_INVALID_ARG);
    // rows too long for 32-bit positions with a step past the end
    EXPECT(hgt_vote_add(f, LLONG_MAX, INT_MAX, q, two, 2, i, 4, f, LLONG_MAX, i, 4, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_vote_add(f, LLONG_MAX, INT_MAX - 1023, q, two, 2, i, 4, f, LLONG_MAX, i, 4, nullptr), HGT_ERR_UNSUPPORTED);

    return abi_check_report("vote_abi_check");
}
