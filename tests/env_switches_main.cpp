// Stand-alone host check of csrc/dkt_env.h (tests/test_env_switches_host.py compiles it with -fsanitize=address,undefined, with and without -DDKT_TWINS, and runs
// it): the snapshot holds copies, follows only dkt_env_reload(), and the three helpers equal the expressions they replaced at the call sites.
#include "dkt_env.h"

#include <cstdio>
#include <string>

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool same(const char* a, const char* b) { return (a == nullptr && b == nullptr) || (a && b && !std::strcmp(a, b)); }

int main() {
    // (all three are PRODUCT switches, so that the program checks the same things in both builds; a VARIANT switch follows at the end)
    const DktSwitch P = DKT_SW_MLL_H2E_MINB, Q = DKT_SW_GRAM_EP_MINB;
    unsetenv("DKT_MLL_H2E_MINB"); unsetenv("DKT_GRAM_EP_MINB"); unsetenv("DKT_GRAM_SPLIT");

    // snapshot, setenv, then reload
    CHECK(dkt_env(P) == nullptr && dkt_env_by_name("MLL_H2E_MINB") == nullptr);
    const unsigned g0 = dkt_env_generation();
    CHECK(g0 != 0);
    setenv("DKT_MLL_H2E_MINB", "17", 1);
    CHECK(dkt_env(P) == nullptr);                                   // not before the reload
    CHECK(dkt_env_generation() == g0);
    dkt_env_reload();
    CHECK(same(dkt_env(P), "17") && same(dkt_env_by_name("MLL_H2E_MINB"), "17") && dkt_env_generation() == g0 + 1);
    CHECK(dkt_env_by_name("DKT_MLL_H2E_MINB") == nullptr && dkt_env_by_name("NO_SUCH_SWITCH") == nullptr && dkt_env_by_name(nullptr) == nullptr);

    // a different variable changes between snapshot and read (each value a fresh heap string that is freed again: a kept getenv() pointer would dangle, and the
    // address sanitizer would see the read)
    const char* held = dkt_env(P);
    for (int i = 0; i < 64; ++i) {
        const std::string big(4096 + 64 * i, 'x');
        setenv("DKT_ENV_TEST_OTHER", big.c_str(), 1);
        setenv("DKT_MLL_H2E_MINB", big.c_str(), 1);                // ... and the variable itself, without a reload
    }
    static char put[] = "DKT_ENV_TEST_PUT=1";
    putenv(put);
    CHECK(same(dkt_env(P), "17") && dkt_env(P) == held);
    unsetenv("DKT_ENV_TEST_OTHER"); unsetenv("DKT_ENV_TEST_PUT");

    // a value longer than the stored length: set, truncated
    dkt_env_reload();
    CHECK(dkt_env(P) && std::strlen(dkt_env(P)) == (size_t)DKT_ENV_VALUE_MAX && std::string(dkt_env(P)) == std::string(DKT_ENV_VALUE_MAX, 'x'));
    const std::string exact(DKT_ENV_VALUE_MAX, '7');
    setenv("DKT_MLL_H2E_MINB", exact.c_str(), 1);
    dkt_env_reload();
    CHECK(same(dkt_env(P), exact.c_str()));

    // an empty value is set; unset after set
    setenv("DKT_MLL_H2E_MINB", "", 1);
    dkt_env_reload();
    CHECK(same(dkt_env(P), "") && dkt_env(Q) == nullptr);
    unsetenv("DKT_MLL_H2E_MINB");
    CHECK(same(dkt_env(P), ""));
    dkt_env_reload();
    CHECK(dkt_env(P) == nullptr);

    // the three helpers against the expressions they replaced, unset and on each value
    CHECK(dkt_env_on(P) == true && dkt_env_is(P, '1') == false && dkt_env_is(P, '2') == false && dkt_env_int(P, 1024) == 1024 && dkt_env_int(P, -1) == -1);
    const char* values[] = {"", "0", "00", "01", "1", "2", "84", "-3"};
    for (const char* s : values) {
        setenv("DKT_MLL_H2E_MINB", s, 1);
        dkt_env_reload();
        const char* v = getenv("DKT_MLL_H2E_MINB");
        CHECK(v && same(dkt_env(P), s));
        CHECK(dkt_env_on(P) == ((v && v[0] == '0') ? 0 : 1));                     // DKT_GRAM_BIG_EP, DKT_MLL_TILED_WDMA, ...
        CHECK(dkt_env_on(P) == !(v && v[0] == '0'));                              // DKT_GRAM_SMALL
        CHECK(dkt_env_is(P, '1') == ((v && v[0] == '1') ? 1 : 0));                // DKT_MLL_F32MFMA, DKT_MLL_TILED_INVRES, DKT_LDS_STAGE_OLD
        CHECK((dkt_env_is(P, '2') ? 2 : 3) == ((v && v[0] == '2') ? 2 : 3));      // DKT_MLL_TILED_WGS
        CHECK(dkt_env_int(P, 1024) == (v ? atoi(v) : 1024));                      // DKT_MLL_H2E_MINB
        CHECK(dkt_env_int(P, -1) == (v ? atoi(v) : -1));                          // DKT_GRAM_SMALL_WG
    }
    setenv("DKT_MLL_H2E_MINB", "0", 1); dkt_env_reload();
    CHECK(!dkt_env_on(P) && !dkt_env_is(P, '1') && dkt_env_int(P, 5) == 0);
    setenv("DKT_MLL_H2E_MINB", "84", 1); dkt_env_reload();
    CHECK(dkt_env_on(P) && !dkt_env_is(P, '2') && dkt_env_int(P, 5) == 84);
    setenv("DKT_MLL_H2E_MINB", "-3", 1); dkt_env_reload();
    CHECK(dkt_env_on(P) && dkt_env_int(P, 5) == -3);
    unsetenv("DKT_MLL_H2E_MINB");

    // a VARIANT switch: read by a twins build only
    setenv("DKT_GRAM_SPLIT", "0", 1);
    dkt_env_reload();
#ifdef DKT_TWINS
    CHECK(same(dkt_env(DKT_SW_GRAM_SPLIT), "0") && same(dkt_env_by_name("GRAM_SPLIT"), "0") && dkt_env_int(DKT_SW_GRAM_SPLIT, 1) == 0);
#else
    CHECK(dkt_env(DKT_SW_GRAM_SPLIT) == nullptr && dkt_env_by_name("GRAM_SPLIT") == nullptr && dkt_env_int(DKT_SW_GRAM_SPLIT, 1) == 1);
#endif
    unsetenv("DKT_GRAM_SPLIT");

    if (failures) return 1;
    std::printf("dkt_env.h OK (%d switches)\n", (int)DKT_SW_COUNT);
    return 0;
}
