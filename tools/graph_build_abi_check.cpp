// Stand-alone host program for the argument checks of the graph-build entry points (hgt_graph_csr_bytes, hgt_graph_csr_build,
// hgt_neighbour_mean_bytes, hgt_neighbour_mean): NULL arrays, negative sizes and strides, id widths other than 4 and 8 bytes, both
// kinds of time at once, sizes beyond 32-bit indices, more CSRs than a table holds, row strides below the row length.  Every call
// returns before a launch, so the program needs no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/graph_build_abi_check.cpp pyhgt_amd/csrc/hgt_graph_build.hip -o graph_build_abi_check \
//         && ./graph_build_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "graph_build_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    std::vector<uint64_t> buf(64, 0);      // host memory behind every pointer: no call may reach a kernel
    void* p = buf.data();
    int32_t* i32 = (int32_t*)buf.data();
    float* f = (float*)buf.data();
    const int64_t big = (int64_t)INT_MAX;   // 2^31 - 1: the first size that is refused
    const int ROW = HGT_GRAPH_TIME_BY_ROW, NBR = HGT_GRAPH_TIME_BY_NBR;

    // ---- scratch size of the CSR build
    uint64_t ws = 0;
    EXPECT(hgt_graph_csr_bytes(-1, &ws), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_bytes(LLONG_MIN, &ws), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_bytes(5, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_bytes(big, &ws), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_graph_csr_bytes(LLONG_MAX, &ws), HGT_ERR_TOO_LARGE);
    uint64_t ws2 = 0;
    EXPECT(hgt_graph_csr_bytes(1000, &ws), HGT_OK);
    CHECK(ws >= 1000 * 36);
    EXPECT(hgt_graph_csr_bytes(2000, &ws2), HGT_OK);
    CHECK(ws2 > ws);
    EXPECT(hgt_graph_csr_bytes(0, &ws2), HGT_OK);
    EXPECT(hgt_graph_csr_bytes(big - 1, &ws2), HGT_OK);

    // ---- the CSR build: every rejection comes before the size query and before a launch
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, -1, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, -4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, -4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, -1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, -2, 8, nullptr, nullptr, ROW, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 2, nullptr, nullptr, ROW, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 0, nullptr, nullptr, ROW, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 16, nullptr, nullptr, ROW, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 4, i32, i32, ROW, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);    // both times
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 4, nullptr, i32, 2, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 4, nullptr, i32, -1, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(nullptr, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, nullptr, 1, 8, nullptr, nullptr, NBR, 5, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, 4, nullptr, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, 4, i32, nullptr, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, 4, i32, i32, nullptr, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, 4, i32, i32, i32, nullptr, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, 4, i32, i32, i32, i32, nullptr, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(nullptr, 1, nullptr, 1, 8, nullptr, nullptr, ROW, 0, 4, 4, nullptr, nullptr, nullptr, i32, p, 1 << 20, nullptr),
           HGT_ERR_INVALID_ARG);                                                                                      // indptr is written even without edges
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 0, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);   // edges, no rows
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, 0, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, big, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 4, nullptr, nullptr, ROW, LLONG_MAX, 4, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, big, 4, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 5, 4, big, i32, i32, i32, i32, p, 1 << 20, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_graph_csr_build(p, 1, p, 1, 8, nullptr, nullptr, ROW, 1000, 4, 4, i32, i32, i32, i32, p, ws - 1, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_graph_csr_build(p, 2, p, 2, 4, nullptr, i32, NBR, 1000, 4, 4, i32, i32, i32, i32, p, 0, nullptr), HGT_ERR_WORKSPACE);

    // ---- scratch size of the mean: host arithmetic only
    uint64_t mb = 1;
    EXPECT(hgt_neighbour_mean_bytes(0, 128, &mb), HGT_OK);
    CHECK(mb >= 256 && mb <= 4096);
    const int64_t C = HGT_GRAPH_MEAN_CHUNK;
    EXPECT(hgt_neighbour_mean_bytes(C - 1, 3, &mb), HGT_OK);
    CHECK(mb <= 4096);                                                     // no row can be longer than a chunk: no partial sums
    uint64_t m1 = 0, m2 = 0;
    EXPECT(hgt_neighbour_mean_bytes(10 * C, 128, &m1), HGT_OK);
    CHECK(m1 >= 20 * 128 * 4);                                             // ten long rows of C + 1 .. 2C - 1 terms: twenty chunks
    EXPECT(hgt_neighbour_mean_bytes(10 * C, 129, &m2), HGT_OK);
    CHECK(m2 > m1);
    EXPECT(hgt_neighbour_mean_bytes(big - 1, 1024, &m2), HGT_OK);
    EXPECT(hgt_neighbour_mean_bytes(-1, 128, &mb), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean_bytes(5, 0, &mb), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean_bytes(5, -3, &mb), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean_bytes(5, 128, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean_bytes(big, 128, &mb), HGT_ERR_TOO_LARGE);

    // ---- the mean
    std::vector<hgt_graph_csr> tab(HGT_SAMPLER_MAX_TRIPLES + 1, hgt_graph_csr{i32, i32});
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 128, 0, 0, 128, f, 128, p, 1 << 20, nullptr), HGT_OK);                  // no rows: nothing to do
    EXPECT(hgt_neighbour_mean(tab.data(), 1, nullptr, 128, 0, 0, 128, nullptr, 128, nullptr, 0, nullptr), HGT_OK);
    EXPECT(hgt_neighbour_mean(nullptr, 1, f, 128, 7, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), 0, f, 128, 7, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), -1, f, 128, 7, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 128, 7, 9, 0, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 127, 7, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);      // ldx < d
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 128, 7, 9, 128, f, 64, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);       // ldo < d
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 128, -7, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 128, 7, -9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), 1, nullptr, 128, 7, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 128, 7, 9, 128, nullptr, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 128, 7, 9, 128, f, 128, nullptr, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), HGT_SAMPLER_MAX_TRIPLES + 1, f, 128, 7, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 128, big, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_TOO_LARGE);
    EXPECT(hgt_neighbour_mean(tab.data(), 1, f, 128, 7, big, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_TOO_LARGE);
    tab[2].indptr = nullptr;
    EXPECT(hgt_neighbour_mean(tab.data(), 3, f, 128, 7, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    tab[2] = hgt_graph_csr{i32, nullptr};
    EXPECT(hgt_neighbour_mean(tab.data(), 3, f, 128, 7, 9, 128, f, 128, p, 1 << 20, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_neighbour_mean(tab.data(), 2, f, 128, 7, 10 * C, 128, f, 128, p, m1 - 1, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_neighbour_mean(tab.data(), 2, f, 128, 7, 9, 128, f, 128, p, 0, nullptr), HGT_ERR_WORKSPACE);

    return abi_check_report("graph_build_abi_check");
}
