// Stand-alone host program for the argument checks of the matcher retrieval entry points (hgt_matcher_topk_bytes, hgt_matcher_topk,
// hgt_matcher_rank): NULL arrays, negative sizes, leading dimensions below d, k outside 1 .. HGT_TOPK_MAX_K, a NaN or infinite scale,
// d outside the supported shapes, sizes of 2^31 - 1 and beyond, scratch that is missing or too small.  Every call is made with host
// pointers and returns before a launch, so the program needs no GPU; it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/matcher_topk_abi_check.cpp pyhgt_amd/csrc/hgt_matcher_topk.hip -o matcher_topk_abi_check \
//         && ./matcher_topk_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "matcher_topk_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <cmath>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    std::vector<int64_t> buf(64, 0);       // host memory behind every pointer: no call may reach a kernel
    int64_t* p = buf.data();
    float* f = (float*)buf.data();
    const int64_t big = (1ll << 31) - 1;    // the first size that is refused
    const int INV = HGT_ERR_INVALID_ARG, UNS = HGT_ERR_UNSUPPORTED, BIG = HGT_ERR_TOO_LARGE, WS = HGT_ERR_WORKSPACE;
    const int K = HGT_TOPK_MAX_K;
    CHECK(K >= 128);

    // ---- the scratch size: host arithmetic only
    uint64_t a = 0, b = 0, c = 0;
    EXPECT(hgt_matcher_topk_bytes(5000, 64, 10, 0, &a), HGT_OK);
    CHECK(a >= 64 * 10 * 8);
    EXPECT(hgt_matcher_topk_bytes(5000, 64, 10, 128, &b), HGT_OK);
    CHECK(b >= 40ull * 64 * 10 * 8);                                  // 40 chunks of 128 rows
    EXPECT(hgt_matcher_topk_bytes(5000, 64, 10, 1, &c), HGT_OK);
    CHECK(c == b);                                                    // chunk_rows is rounded up to the rows of one step
    EXPECT(hgt_matcher_topk_bytes(0, 64, K, 0, &c), HGT_OK);
    EXPECT(hgt_matcher_topk_bytes(5000, 0, 1, 0, &c), HGT_OK);
    EXPECT(hgt_matcher_topk_bytes(big - 1, 256, K, 0, &c), HGT_OK);
    EXPECT(hgt_matcher_topk_bytes(5000, big - 1, 1, 0, &c), HGT_OK);
    EXPECT(hgt_matcher_topk_bytes(5000, 64, 10, 0, nullptr), INV);
    EXPECT(hgt_matcher_topk_bytes(-1, 64, 10, 0, &c), INV);
    EXPECT(hgt_matcher_topk_bytes(5000, -1, 10, 0, &c), INV);
    EXPECT(hgt_matcher_topk_bytes(5000, 64, 0, 0, &c), INV);
    EXPECT(hgt_matcher_topk_bytes(5000, 64, -3, 0, &c), INV);
    EXPECT(hgt_matcher_topk_bytes(5000, 64, 10, -1, &c), INV);
    EXPECT(hgt_matcher_topk_bytes(5000, 64, K + 1, 0, &c), UNS);
    EXPECT(hgt_matcher_topk_bytes(5000, 64, INT_MAX, 0, &c), UNS);
    EXPECT(hgt_matcher_topk_bytes(5000, big, 10, 0, &c), UNS);
    EXPECT(hgt_matcher_topk_bytes(5000, LLONG_MAX, 10, 0, &c), UNS);
    EXPECT(hgt_matcher_topk_bytes(big, 64, 10, 0, &c), BIG);
    EXPECT(hgt_matcher_topk_bytes(1ll << 31, 64, 10, 0, &c), BIG);
    EXPECT(hgt_matcher_topk_bytes(LLONG_MAX, 64, 10, 0, &c), BIG);
    EXPECT(hgt_matcher_topk_bytes(big - 1, big - 1, K, 128, &c), BIG);  // the chunks' lists would pass every buffer

    // ---- top-k: (tx, ld_x, n_cand, ty, ld_y, n_query, d, scale, k, chunk_rows, values, indices, ws, ws_bytes, stream)
#define TOPK(tx, ldx, N, ty, ldy, Q, d, scale, k, rows, val, idx, ws, bytes) \
    hgt_matcher_topk(tx, ldx, N, ty, ldy, Q, d, scale, k, rows, val, idx, ws, bytes, nullptr)
    EXPECT(TOPK(f, 64, 5000, f, 64, 0, 64, 0.125f, 10, 0, f, p, p, a), HGT_OK);            // no query: nothing to do, no launch
    EXPECT(TOPK(f, 64, 5000, nullptr, 64, 0, 64, 0.125f, 10, 0, nullptr, nullptr, nullptr, 0), HGT_OK);
    EXPECT(TOPK(nullptr, 64, 5000, f, 64, 64, 64, 0.125f, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, nullptr, 64, 64, 64, 0.125f, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, 10, 0, nullptr, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, 10, 0, f, nullptr, p, a), INV);
    EXPECT(TOPK(f, 64, -1, f, 64, 64, 64, 0.125f, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, -1, 64, 0.125f, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, -4, 0.125f, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 63, 5000, f, 64, 64, 64, 0.125f, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 60, 64, 64, 0.125f, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, 0, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, -1, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, 10, -1, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, NAN, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, INFINITY, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, -INFINITY, 10, 0, f, p, p, a), INV);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, K + 1, 0, f, p, p, a), UNS);
    EXPECT(TOPK(f, 66, 5000, f, 66, 64, 66, 0.125f, 10, 0, f, p, p, a), UNS);               // d % 4
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 0, 0.125f, 10, 0, f, p, p, a), UNS);
    EXPECT(TOPK(f, 1028, 5000, f, 1028, 64, 1028, 0.125f, 10, 0, f, p, p, a), UNS);
    EXPECT(TOPK(f, 64, 5000, f, 64, big, 64, 0.125f, 10, 0, f, p, p, a), UNS);
    EXPECT(TOPK(f, 64, big, f, 64, 64, 64, 0.125f, 10, 0, f, p, p, a), BIG);
    EXPECT(TOPK(f, 64, LLONG_MAX, f, 64, 64, 64, 0.125f, 10, 0, f, p, p, a), BIG);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, 10, 0, f, p, nullptr, a), WS);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, 10, 0, f, p, p, a - 1), WS);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, 10, 0, f, p, p, 0), WS);
    EXPECT(TOPK(f, 64, 5000, f, 64, 64, 64, 0.125f, 10, 128, f, p, p, a), WS);              // more chunks need more than the default's scratch
    EXPECT(TOPK(nullptr, 64, 0, f, 64, 64, 64, 0.125f, 10, 0, f, p, nullptr, 0), WS);       // even the padding-only call owns its scratch

    // ---- ranks: (tx, ld_x, n_cand, ty, ld_y, n_query, d, scale, chunk_rows, index, rank, ws, ws_bytes, stream)
#define RANK(tx, ldx, N, ty, ldy, Q, d, scale, rows, idx, out, ws, bytes) \
    hgt_matcher_rank(tx, ldx, N, ty, ldy, Q, d, scale, rows, idx, out, ws, bytes, nullptr)
    uint64_t r = 0;
    EXPECT(hgt_matcher_topk_bytes(5000, 64, 1, 0, &r), HGT_OK);
    EXPECT(RANK(f, 64, 5000, f, 64, 0, 64, 0.125f, 0, p, p, p, r), HGT_OK);
    EXPECT(RANK(nullptr, 64, 5000, f, 64, 64, 64, 0.125f, 0, p, p, p, r), INV);
    EXPECT(RANK(f, 64, 5000, nullptr, 64, 64, 64, 0.125f, 0, p, p, p, r), INV);
    EXPECT(RANK(f, 64, 5000, f, 64, 64, 64, 0.125f, 0, nullptr, p, p, r), INV);
    EXPECT(RANK(f, 64, 5000, f, 64, 64, 64, 0.125f, 0, p, nullptr, p, r), INV);
    EXPECT(RANK(f, 64, -1, f, 64, 64, 64, 0.125f, 0, p, p, p, r), INV);
    EXPECT(RANK(f, 64, 5000, f, 64, -1, 64, 0.125f, 0, p, p, p, r), INV);
    EXPECT(RANK(f, 60, 5000, f, 64, 64, 64, 0.125f, 0, p, p, p, r), INV);
    EXPECT(RANK(f, 64, 5000, f, 64, 64, 64, 0.125f, -1, p, p, p, r), INV);
    EXPECT(RANK(f, 64, 5000, f, 64, 64, 64, NAN, 0, p, p, p, r), INV);
    EXPECT(RANK(f, 66, 5000, f, 66, 64, 66, 0.125f, 0, p, p, p, r), UNS);
    EXPECT(RANK(f, 2048, 5000, f, 2048, 64, 2048, 0.125f, 0, p, p, p, r), UNS);
    EXPECT(RANK(f, 64, 5000, f, 64, big, 64, 0.125f, 0, p, p, p, r), UNS);
    EXPECT(RANK(f, 64, big, f, 64, 64, 64, 0.125f, 0, p, p, p, r), BIG);
    EXPECT(RANK(f, 64, 5000, f, 64, 64, 64, 0.125f, 0, p, p, nullptr, r), WS);
    EXPECT(RANK(f, 64, 5000, f, 64, 64, 64, 0.125f, 0, p, p, p, r - 1), WS);
    EXPECT(RANK(f, 64, 5000, f, 64, 64, 64, 0.125f, 128, p, p, p, r), WS);

    return abi_check_report("matcher_topk_abi_check");
}
