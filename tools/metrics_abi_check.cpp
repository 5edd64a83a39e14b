// Stand-alone host program for the argument checks of the task-metric entry points (hgt_rank_metrics, hgt_segment_first_nll,
// hgt_segment_first_nll_bwd): sizes at the ends of their ranges, NULL arrays, both relevance forms at once, leading dimensions below
// the row length.  Every call returns before a launch, so the program needs no GPU; it is meant to be built with the host sanitizers
// and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/metrics_abi_check.cpp pyhgt_amd/csrc/hgt_task_metrics.hip -o metrics_abi_check \
//         && ./metrics_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "metrics_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    std::vector<uint64_t> buf(64, 0);      // host memory behind every pointer: no call may reach a kernel
    float* f = (float*)buf.data();
    double* d = (double*)buf.data();
    const int64_t* q = (const int64_t*)buf.data();

    // ranks: nothing to do
    EXPECT(hgt_rank_metrics(nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_rank_metrics(f, f, nullptr, nullptr, 0, 8, 8, 8, 3, d, d, nullptr), HGT_OK);
    EXPECT(hgt_rank_metrics(nullptr, nullptr, nullptr, q, 0, INT_MAX, -5, -5, INT_MAX, nullptr, nullptr, nullptr), HGT_OK);
    // negative sizes, before anything else
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, -1, 8, 8, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, INT_MIN, 8, 8, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, -1, 8, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, INT_MIN, 8, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, 8, 8, 0, -1, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 0, 8, 8, 0, INT_MIN, d, d, nullptr), HGT_ERR_INVALID_ARG);
    // both relevance forms, even without a row
    EXPECT(hgt_rank_metrics(f, f, q, nullptr, 2, 8, 8, 8, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, f, q, nullptr, 0, 8, 8, 8, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    // NULL arrays with rows
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, 8, 8, 0, 0, nullptr, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, 8, 8, 0, 0, d, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(nullptr, nullptr, nullptr, nullptr, 2, 8, 8, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(nullptr, nullptr, nullptr, q, 2, 8, 0, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    // leading dimensions below the row length (regular rows only: ragged rows do not read them)
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, 8, 7, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, 8, -8, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, 8, LLONG_MIN, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, f, nullptr, nullptr, 2, 8, 8, 7, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_rank_metrics(f, f, nullptr, nullptr, 2, 8, 8, LLONG_MIN, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);
    // rows too long for 32-bit positions with a tile past the end
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, INT_MAX, LLONG_MAX, 0, 0, d, d, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, q, 2, INT_MAX - 1023, 0, 0, 0, d, d, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, INT_MAX, INT_MAX, 0, 0, INT_MAX, d, d, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_rank_metrics(f, nullptr, nullptr, nullptr, 2, INT_MAX - 1024, INT_MAX - 1025, 0, 0, d, d, nullptr), HGT_ERR_INVALID_ARG);

    // the loss, forward
    EXPECT(hgt_segment_first_nll(nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_segment_first_nll(nullptr, nullptr, 0, INT_MAX, nullptr, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_segment_first_nll(f, q, -1, 8, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll(f, q, INT_MIN, 8, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll(f, q, 0, -1, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll(f, q, 3, INT_MIN, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll(f, q, 3, 0, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll(f, q, 3, 1, f, f, nullptr), HGT_ERR_INVALID_ARG);       // no segment of two entries fits
    EXPECT(hgt_segment_first_nll(nullptr, q, 3, 8, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll(f, nullptr, 3, 8, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll(f, q, 3, 8, nullptr, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll(f, q, INT_MAX, INT_MAX, f, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    // and backward
    EXPECT(hgt_segment_first_nll_bwd(nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_segment_first_nll_bwd(f, q, -1, 8, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll_bwd(f, q, 3, -1, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll_bwd(f, q, 3, 1, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll_bwd(nullptr, q, 3, 8, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll_bwd(f, nullptr, 3, 8, f, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll_bwd(f, q, 3, 8, nullptr, f, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll_bwd(f, q, 3, 8, f, nullptr, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_segment_first_nll_bwd(f, q, INT_MAX, INT_MAX, f, f, nullptr, nullptr), HGT_ERR_INVALID_ARG);

    return abi_check_report("metrics_abi_check");
}
