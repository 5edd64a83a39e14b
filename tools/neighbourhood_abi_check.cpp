// Stand-alone host program for the argument checks of the neighbourhood entry points (hgt_nb_constants, hgt_nb_sort_bytes,
// hgt_nb_seeds, hgt_nb_number, hgt_nb_expand, hgt_nb_fill, hgt_nb_finish, hgt_nb_reset): NULL tables and heads, table sizes outside the
// sampler's limits, negative sizes and sizes of 2^31 - 1 and beyond, NULL arrays where the sizes say they are read or written, type
// ranges outside their level, triple types outside the table, sort scratch that is too small.  Every call returns before a launch,
// so the program needs no GPU (without one hgt_nb_sort_bytes answers HGT_ERR_LAUNCH, as documented, and the one case that needs its
// answer -- a scratch 256 bytes short -- is left out with a note; a scratch below 256 bytes is refused everywhere); it is meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/neighbourhood_abi_check.cpp pyhgt_amd/csrc/hgt_neighbourhood.hip -o neighbourhood_abi_check \
//         && ./neighbourhood_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "neighbourhood_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    std::vector<int64_t> buf(64, 0);       // host memory behind every pointer: no call may reach a kernel
    int64_t* p = buf.data();
    uint64_t* u = (uint64_t*)buf.data();
    int32_t* i32 = (int32_t*)buf.data();
    float* f = (float*)buf.data();
    std::vector<hgt_nb_type> types(4);
    std::vector<hgt_nb_triple> tri(3);
    for (int m = 0; m < 3; ++m) { tri[m].tgt_type = m % 2; tri[m].src_type = 1 - m % 2; tri[m].rel_id = m; }
    const hgt_nb_type* ty = types.data();
    const hgt_nb_triple* tr = tri.data();
    const int64_t big = (1ll << 31) - 1;    // the first size that is refused
    const int32_t MT = HGT_SAMPLER_MAX_TRIPLES, MY = HGT_SAMPLER_MAX_TYPES;
    const int INV = HGT_ERR_INVALID_ARG;
    std::vector<int64_t> tb{0, 3}, te{3, 5};           // a level of 5 rows: 3 of type 0, 2 of type 1

    // ---- constants and struct sizes
    int32_t chunk = 0, wave = 0, words = 0;
    EXPECT(hgt_nb_constants(&chunk, &wave, &words), HGT_OK);
    CHECK(chunk == HGT_NB_CHUNK && wave == HGT_NB_WAVE_ROWS && words == HGT_NB_HEAD_WORDS);
    EXPECT(hgt_nb_constants(nullptr, &wave, &words), INV);
    EXPECT(hgt_nb_constants(&chunk, nullptr, &words), INV);
    EXPECT(hgt_nb_constants(&chunk, &wave, nullptr), INV);
    CHECK(sizeof(hgt_nb_type) == 40 && sizeof(hgt_nb_triple) == 72);
    CHECK(HGT_NB_HEAD_TYPE_BEGIN + MY <= HGT_NB_HEAD_TYPE_END && HGT_NB_HEAD_TYPE_END + MY <= HGT_NB_HEAD_WORDS);

    // ---- the sort scratch: no launch (rocPRIM's size query)
    uint64_t a = 0, b = 0;
    const int query = hgt_nb_sort_bytes(5000, 4, &a);
    const bool answered = query == HGT_OK;  // rocPRIM picks its configuration by the device's architecture: no device, no answer
    if (answered) {
        CHECK(a >= 256);
        EXPECT(hgt_nb_sort_bytes(0, 1, &b), HGT_OK);
    } else {
        CHECK(query == HGT_ERR_LAUNCH);
        a = 1 << 20;
        std::printf("note: no device answers rocPRIM's size query (HGT_ERR_LAUNCH): the one HGT_ERR_WORKSPACE case that needs its answer "
                    "(a scratch 256 bytes short) is not run\n");
    }
    EXPECT(hgt_nb_sort_bytes(5000, 4, nullptr), INV);
    EXPECT(hgt_nb_sort_bytes(-1, 4, &b), INV);
    EXPECT(hgt_nb_sort_bytes(big, 4, &b), INV);
    EXPECT(hgt_nb_sort_bytes(LLONG_MAX, 4, &b), INV);
    EXPECT(hgt_nb_sort_bytes(5000, 0, &b), INV);
    EXPECT(hgt_nb_sort_bytes(5000, MY + 1, &b), INV);

    // ---- seeds: (types, T, seed_type, seed_id, S, cand, head, stream)
    EXPECT(hgt_nb_seeds(nullptr, 2, i32, p, 5, u, p, nullptr), INV);
    EXPECT(hgt_nb_seeds(ty, 0, i32, p, 5, u, p, nullptr), INV);
    EXPECT(hgt_nb_seeds(ty, MY + 1, i32, p, 5, u, p, nullptr), INV);
    EXPECT(hgt_nb_seeds(ty, 2, i32, p, 5, u, nullptr, nullptr), INV);
    EXPECT(hgt_nb_seeds(ty, 2, i32, p, -1, u, p, nullptr), INV);
    EXPECT(hgt_nb_seeds(ty, 2, i32, p, big, u, p, nullptr), INV);
    EXPECT(hgt_nb_seeds(ty, 2, nullptr, p, 5, u, p, nullptr), INV);
    EXPECT(hgt_nb_seeds(ty, 2, i32, nullptr, 5, u, p, nullptr), INV);
    EXPECT(hgt_nb_seeds(ty, 2, i32, p, 5, nullptr, p, nullptr), INV);

    // ---- number: (types, T, triples, M, cand, cap, keys_out, sort_tmp, sort_bytes, row_base, expand, order, node_type, row_id, head, stream)
#define NUMBER(ty, T, tr, M, cand, cap, keys, tmp, bytes, base, o, nt, id, head) \
    hgt_nb_number(ty, T, tr, M, cand, cap, keys, tmp, bytes, base, 1, o, nt, id, head, nullptr)
    EXPECT(NUMBER(nullptr, 2, tr, 3, u, 5000, u, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 0, tr, 3, u, 5000, u, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, nullptr, 3, u, 5000, u, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, -1, u, 5000, u, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, MT + 1, u, 5000, u, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 0, u, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, -5, u, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, big, u, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, a, -1, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, a, big - 5000, p, p, p, p), INV);       // the last row's number would not fit
    EXPECT(NUMBER(ty, 2, tr, 3, nullptr, 5000, u, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, nullptr, p, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, nullptr, a, 0, p, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, a, 0, nullptr, p, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, a, 0, p, nullptr, p, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, a, 0, p, p, nullptr, p), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, a, 0, p, p, p, nullptr), INV);
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, 0, 0, p, p, p, p), HGT_ERR_WORKSPACE);          // refused before the size query
    EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, 255, 0, p, p, p, p), HGT_ERR_WORKSPACE);
    if (answered) EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, a - 256, 0, p, p, p, p), HGT_ERR_WORKSPACE);
    else EXPECT(NUMBER(ty, 2, tr, 3, u, 5000, u, p, a, 0, p, p, p, p), HGT_ERR_LAUNCH);                // documented: no device, no answer

    // ---- expand: (types, T, triples_dev, triples_host, M, keys, type_begin, type_end, n_level, n_chunks, has_max_time, max_time,
    //      item_chunks, item_entries, chunk_cnt, cand, capacity, head, stream)
#define EXPAND(ty, T, trd, trh, M, keys, tb, te, n, chunks, ic, ie, cc, cand, cap, head) \
    hgt_nb_expand(ty, T, trd, trh, M, keys, tb, te, n, chunks, 1, 2001, ic, ie, cc, cand, cap, head, nullptr)
    EXPECT(EXPAND(nullptr, 2, tr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, nullptr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, nullptr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, nullptr, te.data(), 5, 9, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), nullptr, 5, 9, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, i32, u, 9000, nullptr), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), -1, 9, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), big, 9, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, -1, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, big, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 4, 9, i32, i32, i32, u, 9000, p), INV);       // type 1 ends behind the level
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, te.data(), tb.data(), 5, 9, i32, i32, i32, u, 9000, p), INV);       // end < begin
    EXPECT(EXPAND(ty, 1, tr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, i32, u, 9000, p), INV);       // a triple type outside the table
    EXPECT(EXPAND(ty, 2, tr, tr, 3, nullptr, tb.data(), te.data(), 5, 9, i32, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, 9, nullptr, i32, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, nullptr, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, nullptr, i32, u, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, i32, nullptr, 9000, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, i32, u, 0, p), INV);          // chunks without room for a claim
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, i32, u, -1, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 3, u, tb.data(), te.data(), 5, 9, i32, i32, i32, u, big, p), INV);
    EXPECT(EXPAND(ty, 2, tr, tr, 0, u, tb.data(), te.data(), 5, 9, i32, i32, i32, u, 9000, p), INV);       // chunks of a graph without triples

    // ---- fill: expand's arguments up to max_time, then (has_time, self_loops, rel_self, row_base, item_chunks, chunk_cnt, src, dst,
    //      edge_type, edge_time, edge_capacity, head, stream)
#define FILL(ty, trh, tb, te, n, chunks, has_time, loops, base, ic, cc, s, d, et, tm, cap, head) \
    hgt_nb_fill(ty, 2, tr, trh, 3, u, tb, te, n, chunks, 1, 2001, has_time, loops, 3, base, ic, cc, s, d, et, tm, cap, head, nullptr)
    EXPECT(FILL(nullptr, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, i32, p, p, p, p, 9005, p), INV);
    EXPECT(FILL(ty, nullptr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, i32, p, p, p, p, 9005, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, i32, p, p, p, p, 9005, nullptr), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 4, 9, 1, 1, 0, i32, i32, p, p, p, p, 9005, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, -1, i32, i32, p, p, p, p, 9005, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, big - 5, i32, i32, p, p, p, p, 9005, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, nullptr, i32, p, p, p, p, 9005, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, nullptr, p, p, p, p, 9005, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, i32, nullptr, p, p, p, 9005, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, i32, p, nullptr, p, p, 9005, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, i32, p, p, nullptr, p, 9005, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, i32, p, p, p, nullptr, 9005, p), INV);     // has_time without edge_time
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 0, 0, 1, 0, i32, i32, nullptr, p, p, nullptr, 5, p), INV);  // loops alone still write
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 0, 0, 1, 0, i32, i32, p, p, p, nullptr, 4, p), INV);        // no room for the loops
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, i32, p, p, p, p, -1, p), INV);
    EXPECT(FILL(ty, tr, tb.data(), te.data(), 5, 9, 1, 1, 0, i32, i32, p, p, p, p, big, p), INV);

    // ---- finish: (types, T, node_type, row_id, n_rows, width, feature_out, seed_type, seed_id, S, out_rows, stream)
    EXPECT(hgt_nb_finish(nullptr, 2, p, p, 5, 3, f, i32, p, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, MY + 1, p, p, 5, 3, f, i32, p, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, nullptr, p, 5, 3, f, i32, p, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, nullptr, 5, 3, f, i32, p, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, p, 5, 3, nullptr, i32, p, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, p, -1, 3, f, i32, p, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, p, big, 3, f, i32, p, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, p, 5, -3, f, i32, p, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, p, 5, 3, f, nullptr, p, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, p, 5, 3, f, i32, nullptr, 2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, p, 5, 3, f, i32, p, 2, nullptr, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, p, 5, 3, f, i32, p, -2, p, nullptr), INV);
    EXPECT(hgt_nb_finish(ty, 2, p, p, 5, 3, f, i32, p, big, p, nullptr), INV);

    // ---- reset: (types, T, keys, n, stream)
    EXPECT(hgt_nb_reset(nullptr, 2, u, 5, nullptr), INV);
    EXPECT(hgt_nb_reset(ty, 0, u, 5, nullptr), INV);
    EXPECT(hgt_nb_reset(ty, 2, nullptr, 5, nullptr), INV);
    EXPECT(hgt_nb_reset(ty, 2, u, -1, nullptr), INV);
    EXPECT(hgt_nb_reset(ty, 2, u, big, nullptr), INV);

    return abi_check_report("neighbourhood_abi_check");
}
