// Stand-alone host program for the argument checks of the seed-trim entry points (hgt_trim_tmp_bytes, hgt_trim_hops, hgt_trim_fill):
// layer counts outside [1, HGT_TRIM_MAX_LAYERS], negative sizes, sizes of 2^31 and beyond, NULL arrays where the sizes say they are
// read or written, scratch that is too small.  Every call returns before a launch, so the program needs no GPU; it is meant to be
// built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/trim_abi_check.cpp pyhgt_amd/csrc/hgt_trim.hip -o trim_abi_check && ./trim_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "trim_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    std::vector<int64_t> buf(64, 0);       // host memory behind every pointer: no call may reach a kernel
    int64_t* p = buf.data();
    int32_t* i32 = (int32_t*)buf.data();
    const int64_t big = 1ll << 31;          // the first size that is refused
    const int32_t ML = HGT_TRIM_MAX_LAYERS;
    const int INV = HGT_ERR_INVALID_ARG;

    // ---- the scratch size: host arithmetic only
    uint64_t a = 0, b = 0;
    EXPECT(hgt_trim_tmp_bytes(1000, 5000, 2, &a), HGT_OK);
    CHECK(a >= 1000 * 4);
    EXPECT(hgt_trim_tmp_bytes(2000, 5000, 2, &b), HGT_OK);
    CHECK(b > a);
    EXPECT(hgt_trim_tmp_bytes(0, 0, 1, &b), HGT_OK);
    EXPECT(hgt_trim_tmp_bytes(big - 1, big - 1, ML, &b), HGT_OK);
    CHECK(ML >= 8);
    EXPECT(hgt_trim_tmp_bytes(1000, 5000, 2, nullptr), INV);
    EXPECT(hgt_trim_tmp_bytes(1000, 5000, 0, &b), INV);
    EXPECT(hgt_trim_tmp_bytes(1000, 5000, -1, &b), INV);
    EXPECT(hgt_trim_tmp_bytes(1000, 5000, ML + 1, &b), INV);
    EXPECT(hgt_trim_tmp_bytes(-1, 5000, 2, &b), INV);
    EXPECT(hgt_trim_tmp_bytes(1000, -1, 2, &b), INV);
    EXPECT(hgt_trim_tmp_bytes(big, 5000, 2, &b), INV);
    EXPECT(hgt_trim_tmp_bytes(1000, big, 2, &b), INV);
    EXPECT(hgt_trim_tmp_bytes(LLONG_MAX, LLONG_MAX, 2, &b), INV);

    // ---- the hop rounds
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, 5000, p, 3, 0, p, a, nullptr), INV);
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, 5000, p, 3, ML + 1, p, a, nullptr), INV);
    EXPECT(hgt_trim_hops(p, 5000, 1, -1, 5000, p, 3, 2, p, a, nullptr), INV);
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, -1, p, 3, 2, p, a, nullptr), INV);
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, 5000, p, -3, 2, p, a, nullptr), INV);
    EXPECT(hgt_trim_hops(p, 5000, 1, big, 5000, p, 3, 2, p, a, nullptr), INV);
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, big, p, 3, 2, p, a, nullptr), INV);
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, 5000, p, big, 2, p, a, nullptr), INV);
    EXPECT(hgt_trim_hops(nullptr, 5000, 1, 1000, 5000, p, 3, 2, p, a, nullptr), INV);          // edges, no edge_index
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, 5000, nullptr, 3, 2, p, a, nullptr), INV);          // seeds, no array
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, 5000, p, 3, 2, nullptr, a, nullptr), INV);
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, 5000, p, 3, 2, p, a - 1, nullptr), HGT_ERR_WORKSPACE);
    EXPECT(hgt_trim_hops(p, 5000, 1, 1000, 5000, p, 3, 2, p, 0, nullptr), HGT_ERR_WORKSPACE);

    // ---- the fill: (edge_index, strides, edge_type, edge_time, node_type, N, E, seeds, n_seeds, L, tmp, tmp_bytes, hop, order, new_id,
    //      edge_order, node_type_out, edge_index_out, edge_type_out, edge_time_out, out_rows, counts, counts_host, stream)
#define FILL(ei, et, tm, nt, N, E, sd, S, L, tmp, bytes, hop, ord, nid, eo, nto, eio, eto, tmo, orow, cnt, host) \
    hgt_trim_fill(ei, 5000, 1, et, tm, nt, N, E, sd, S, L, tmp, bytes, hop, ord, nid, eo, nto, eio, eto, tmo, orow, cnt, host, nullptr)
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 0, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, ML + 1, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, -1, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, -1, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, -3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, big, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, big, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(nullptr, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, nullptr, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, nullptr, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, nullptr, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, nullptr, a, i32, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, nullptr, p, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, nullptr, p, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, nullptr, p, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, nullptr, p, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, nullptr, p, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, p, nullptr, p, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, nullptr, p, p, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, p, nullptr, p, i32, p), INV);   // edge_time without its output
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, nullptr, i32, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, nullptr, p), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a, i32, p, p, p, p, p, p, p, p, i32, nullptr), INV);
    EXPECT(FILL(p, p, p, p, 1000, 5000, p, 3, 2, p, a - 1, i32, p, p, p, p, p, p, p, p, i32, p), HGT_ERR_WORKSPACE);

    return abi_check_report("trim_abi_check");
}
