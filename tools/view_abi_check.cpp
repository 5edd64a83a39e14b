// Stand-alone host program for the argument checks of the whole-graph view entry points (hgt_view_tmp_bytes, hgt_view_build): negative
// sizes, sizes of 2^31 - 1 and beyond, table sizes outside the sampler's limits, NULL arrays where the sizes say they are read or
// written, an edge_index without its companions or with a short stride, scratch that is missing or too small.  Every call returns
// before a launch, so the program needs no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/view_abi_check.cpp pyhgt_amd/csrc/hgt_graph_view.hip -o view_abi_check && ./view_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "view_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    std::vector<int64_t> buf(64, 0);       // host memory behind every pointer: no call may reach a kernel
    int64_t* p = buf.data();
    int32_t* i32 = (int32_t*)buf.data();
    std::vector<hgt_view_triple> table(4);
    const hgt_view_triple* tab = table.data();
    const int64_t big = (1ll << 31) - 1;    // the first size that is refused
    const int32_t MT = HGT_SAMPLER_MAX_TRIPLES;
    const int INV = HGT_ERR_INVALID_ARG;

    // ---- the scratch size: host arithmetic only
    uint64_t a = 0, b = 0;
    EXPECT(hgt_view_tmp_bytes(5000, &a), HGT_OK);
    CHECK(a >= (5000 / HGT_VIEW_TILE + 1) * 4);
    EXPECT(hgt_view_tmp_bytes(5000000, &b), HGT_OK);
    CHECK(b > a);
    EXPECT(hgt_view_tmp_bytes(0, &b), HGT_OK);
    CHECK(b >= 4);
    EXPECT(hgt_view_tmp_bytes(big - 1, &b), HGT_OK);
    EXPECT(hgt_view_tmp_bytes(5000, nullptr), INV);
    EXPECT(hgt_view_tmp_bytes(-1, &b), INV);
    EXPECT(hgt_view_tmp_bytes(big, &b), INV);
    EXPECT(hgt_view_tmp_bytes(1ll << 31, &b), INV);
    EXPECT(hgt_view_tmp_bytes(LLONG_MAX, &b), INV);
    CHECK(sizeof(hgt_view_triple) == 80);

    // ---- the build: (table, n_triples, n_relations, n_entries, filtered, has_max_time, max_time, has_time, src32, dst32, time32,
    //      edge_index, edge_index_stride, edge_type, edge_time, rel_ptr, tmp, tmp_bytes, head_host, stream)
#define BUILD(tab, M, R, E, filt, has_time, s32, d32, t32, ei, stride, et, tm, rp, tmp, bytes) \
    hgt_view_build(tab, M, R, E, filt, 1, 2001, has_time, s32, d32, t32, ei, stride, et, tm, rp, tmp, bytes, p, nullptr)
    EXPECT(BUILD(tab, 3, 4, -1, 1, 1, i32, i32, i32, p, 5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, 3, 4, big, 1, 1, i32, i32, i32, p, big, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, 3, 4, 1ll << 31, 1, 1, i32, i32, i32, p, 1ll << 31, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, 3, 4, LLONG_MAX, 1, 1, i32, i32, i32, p, LLONG_MAX, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, -1, 4, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, MT + 1, 4, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, 3, 0, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, 3, -2, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, 3, MT + 2, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(nullptr, 3, 4, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(nullptr, 0, 1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, i32, nullptr, 0), INV);   // even the empty view has a table
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, nullptr, i32, i32, p, 5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, nullptr, i32, p, 5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, i32, nullptr, p, 5000, p, p, i32, p, a), INV);        // has_time without time32
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, i32, i32, p, 5000, nullptr, p, i32, p, a), INV);      // edge_index without edge_type
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, i32, i32, p, 5000, p, nullptr, i32, p, a), INV);      // ... without edge_time under has_time
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, i32, i32, p, 4999, p, p, i32, p, a), INV);            // rows of edge_index would overlap
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, i32, i32, p, -5000, p, p, i32, p, a), INV);
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, nullptr, p, a), INV);
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, i32, nullptr, a), INV);      // a filtered build needs its scratch
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 0, i32, i32, nullptr, p, 5000, p, nullptr, i32, nullptr, a), INV);
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, i32, p, a - 256), HGT_ERR_WORKSPACE);
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 1, i32, i32, i32, p, 5000, p, p, i32, p, 0), HGT_ERR_WORKSPACE);
    EXPECT(BUILD(tab, 3, 4, 5000, 1, 0, i32, i32, nullptr, nullptr, 0, nullptr, nullptr, i32, p, 3), HGT_ERR_WORKSPACE);

    return abi_check_report("view_abi_check");
}
