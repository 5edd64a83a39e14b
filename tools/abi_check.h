// What the tools/*_abi_check.cpp programs share: the failure counter, EXPECT (a call returns the documented code), CHECK (a host
// condition holds) and the closing report line.  `make -C pyhgt_amd/csrc abicheck` builds them all with the host sanitizers and runs
// each on the CPU; the single build line stands in each program's comment.
#pragma once
#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define EXPECT(call, code)                                                                        \
    do {                                                                                          \
        const int rc_ = (call);                                                                   \
        if (rc_ != (code)) {                                                                      \
            std::printf("line %d: %s returned %d, expected %d\n", __LINE__, #call, rc_, (code)); \
            ++failures;                                                                           \
        }                                                                                         \
    } while (0)
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("line %d: %s is false\n", __LINE__, #cond);   \
            ++failures;                                                \
        }                                                              \
    } while (0)

// the last statement of main: "<name>: ok" and exit status 0, or the number of failed lines
static inline int abi_check_report(const char* name) {
    if (failures) std::printf("%s: %d FAILED\n", name, failures);
    else std::printf("%s: ok\n", name);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
