// Stand-alone host program for the argument checks of the optimizer entry points (hgt_optim_chunk_table, hgt_optim_tables_bytes,
// hgt_grad_sqnorm, hgt_grad_norm_join, hgt_adamw_step): negative sizes, NULL tables, no tensor or group with chunks, more chunks than a
// grid dimension holds, a negative or NaN max_norm -- and the host-side chunk table itself: every element in exactly one chunk, no
// chunk across two tensors, chunks in tensor order.  Every device call returns before a launch, so the program needs no GPU; it is
// meant to be built with the host sanitizers and run on its own:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ipyhgt_amd/csrc tools/optim_abi_check.cpp pyhgt_amd/csrc/hgt_optim.hip -o optim_abi_check && ./optim_abi_check
//
// (`make -C pyhgt_amd/csrc abicheck` builds and runs all the *_abi_check programs this way; it reads the .hip names from the line above.)
// Exit status 0 and "optim_abi_check: ok" = every call returned the documented code and the sanitizers found nothing.
#include <climits>
#include <cmath>
#include <vector>

#include "abi_check.h"
#include "hgt_hip.h"

int main() {
    std::vector<uint64_t> buf(64, 0);      // host memory behind every pointer: no call may reach a kernel
    const hgt_optim_tensor* T = (const hgt_optim_tensor*)buf.data();
    const hgt_optim_group* G = (const hgt_optim_group*)buf.data();
    const hgt_optim_chunk* Ch = (const hgt_optim_chunk*)buf.data();
    double* d = (double*)buf.data();
    float* f = (float*)buf.data();
    const int64_t big = (int64_t)INT_MAX + 1;

    // ---- the chunk table
    int32_t chunk = 0;
    EXPECT(hgt_optim_constants(&chunk), HGT_OK);
    CHECK(chunk == HGT_OPTIM_CHUNK);
    EXPECT(hgt_optim_constants(nullptr), HGT_ERR_INVALID_ARG);
    const int64_t C = HGT_OPTIM_CHUNK;
    const std::vector<int64_t> numel = {1, 3, 4, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5, 0, 7};
    int64_t n = -1;
    EXPECT(hgt_optim_chunk_table(numel.data(), (int32_t)numel.size(), nullptr, 0, &n), HGT_OK);
    CHECK(n == 6 + 1 + 1 + 2 + 3 + 0 + 1);
    std::vector<hgt_optim_chunk> table((size_t)n + 1);
    table[(size_t)n].row = -77;                                                   // one entry past the table: must survive
    int64_t m = -1;
    EXPECT(hgt_optim_chunk_table(numel.data(), (int32_t)numel.size(), table.data(), n, &m), HGT_OK);
    CHECK(m == n && table[(size_t)n].row == -77);
    {
        int64_t c = 0;
        for (int32_t r = 0; r < (int32_t)numel.size(); ++r) {
            for (int64_t first = 0; first < numel[r]; first += C, ++c) {
                CHECK(c < n && table[(size_t)c].row == r && table[(size_t)c].first == first);
            }
        }
        CHECK(c == n);
    }
    EXPECT(hgt_optim_chunk_table(numel.data(), (int32_t)numel.size(), table.data(), n - 1, &m), HGT_ERR_WORKSPACE);
    EXPECT(hgt_optim_chunk_table(numel.data(), (int32_t)numel.size(), table.data(), -1, &m), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_chunk_table(numel.data(), -1, nullptr, 0, &m), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_chunk_table(numel.data(), INT_MIN, nullptr, 0, &m), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_chunk_table(nullptr, 3, nullptr, 0, &m), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_chunk_table(numel.data(), 3, nullptr, 0, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_chunk_table(nullptr, 0, nullptr, 0, &m), HGT_OK);
    CHECK(m == 0);
    const std::vector<int64_t> bad = {5, -1, 7}, huge = {LLONG_MAX, 4}, many = {C * (int64_t)INT_MAX, 1};
    EXPECT(hgt_optim_chunk_table(bad.data(), 3, nullptr, 0, &m), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_chunk_table(huge.data(), 2, nullptr, 0, &m), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_optim_chunk_table(many.data(), 2, nullptr, 0, &m), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_optim_chunk_table(many.data(), 1, nullptr, 0, &m), HGT_OK);
    CHECK(m == INT_MAX);

    // ---- sizes
    uint64_t a = 1, b = 1, c = 1, e = 1;
    EXPECT(hgt_optim_tables_bytes(0, 0, 0, &a, &b, &c, &e), HGT_OK);
    CHECK(a == 0 && b == 0 && c == 0 && e == 0);
    EXPECT(hgt_optim_tables_bytes(198, 2, 5300, &a, &b, &c, &e), HGT_OK);
    CHECK(b == 198 * sizeof(hgt_optim_tensor) && a == b + 2 * sizeof(hgt_optim_group) && c == 5300 * sizeof(hgt_optim_chunk) && e == 5300 * 8);
    EXPECT(hgt_optim_tables_bytes(INT_MAX, INT_MAX, INT_MAX, &a, &b, &c, &e), HGT_OK);
    EXPECT(hgt_optim_tables_bytes(-1, 2, 5, &a, &b, &c, &e), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_tables_bytes(1, -2, 5, &a, &b, &c, &e), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_tables_bytes(1, 2, -5, &a, &b, &c, &e), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_tables_bytes(1, 2, LLONG_MIN, &a, &b, &c, &e), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_tables_bytes(1, 2, big, &a, &b, &c, &e), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_optim_tables_bytes(1, 2, 5, nullptr, &b, &c, &e), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_tables_bytes(1, 2, 5, &a, nullptr, &c, &e), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_tables_bytes(1, 2, 5, &a, &b, nullptr, &e), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_optim_tables_bytes(1, 2, 5, &a, &b, &c, nullptr), HGT_ERR_INVALID_ARG);

    // ---- the squared norm: nothing to do, then every rejection
    EXPECT(hgt_grad_sqnorm(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_grad_sqnorm(T, 3, G, 1, Ch, 0, nullptr, nullptr), HGT_OK);
    EXPECT(hgt_grad_sqnorm(T, -1, G, 1, Ch, 0, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(T, 3, G, -1, Ch, 0, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(T, 3, G, 1, Ch, -1, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(T, 3, G, 1, Ch, LLONG_MIN, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(nullptr, 3, G, 1, Ch, 4, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(T, 3, nullptr, 1, Ch, 4, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(T, 3, G, 1, nullptr, 4, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(T, 3, G, 1, Ch, 4, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(T, 0, G, 1, Ch, 4, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(T, 3, G, 0, Ch, 4, d, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_sqnorm(T, 3, G, 1, Ch, big, d, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_grad_sqnorm(T, 3, G, 1, Ch, LLONG_MAX, d, nullptr), HGT_ERR_UNSUPPORTED);

    // ---- the join (it launches even without a chunk, so only its rejections can be called here)
    EXPECT(hgt_grad_norm_join(d, -1, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_norm_join(d, LLONG_MIN, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_norm_join(d, 4, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_norm_join(nullptr, 0, nullptr, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_norm_join(nullptr, 4, f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_grad_norm_join(d, big, f, nullptr), HGT_ERR_UNSUPPORTED);

    // ---- the update
    EXPECT(hgt_adamw_step(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0.0f, nullptr), HGT_OK);
    EXPECT(hgt_adamw_step(T, 3, G, 1, Ch, 0, f, 0.5f, nullptr), HGT_OK);
    EXPECT(hgt_adamw_step(T, 3, G, 1, Ch, 0, nullptr, -1.0f, nullptr), HGT_OK);                       // max_norm is not read without a norm
    EXPECT(hgt_adamw_step(T, -1, G, 1, Ch, 0, f, 0.5f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 3, G, -1, Ch, 0, f, 0.5f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 3, G, 1, Ch, -1, f, 0.5f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(nullptr, 3, G, 1, Ch, 4, f, 0.5f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 3, nullptr, 1, Ch, 4, f, 0.5f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 3, G, 1, nullptr, 4, f, 0.5f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 0, G, 1, Ch, 4, f, 0.5f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 3, G, 0, Ch, 4, f, 0.5f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 3, G, 1, Ch, 4, f, -0.5f, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 3, G, 1, Ch, 4, f, NAN, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 3, G, 1, Ch, 0, f, NAN, nullptr), HGT_ERR_INVALID_ARG);
    EXPECT(hgt_adamw_step(T, 3, G, 1, Ch, big, f, 0.5f, nullptr), HGT_ERR_UNSUPPORTED);
    EXPECT(hgt_adamw_step(T, 3, G, 1, Ch, big, nullptr, 0.0f, nullptr), HGT_ERR_UNSUPPORTED);

    return abi_check_report("optim_abi_check");
}
