// dkt_env.h -- the accessors of dkt_switches.def: ONE snapshot of the environment switches per library, taken at the first read and again at dkt_env_reload()
// (= dkt_reload_env() / dkt_x16_reload_env() of the ABI headers: tests and A/B tools flip switches inside one process).  Header-only, host-only, no HIP header.
//
// The snapshot holds COPIES of the values: Python's `os.environ[...] = ...` calls putenv() between two library calls, after which a pointer that getenv() returned
// earlier may dangle.  A copy keeps at most DKT_ENV_VALUE_MAX characters; a longer value counts as set and is truncated (every switch is a small integer).
// Defaults and interpretations live at the call sites (they differ by call site on purpose), through the three helpers at the end.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

enum DktSwitch {
#define X(name, cls) DKT_SW_##name,
#include "dkt_switches.def"
#undef X
    DKT_SW_COUNT
};

constexpr int DKT_ENV_VALUE_MAX = 31;
// (hidden: each shared object keeps its own snapshot, and a twins build never shares these functions with a product build loaded into the same process)
#define DKT_ENV_FN inline __attribute__((visibility("hidden")))

// A VARIANT switch has no name outside a -DDKT_TWINS build: the product reads none of them and its binary contains none of their names (tests/test_abi_host.py).
#define DKT_ENV_NAME_PRODUCT(name) "DKT_" #name
#ifdef DKT_TWINS
#define DKT_ENV_NAME_VARIANT(name) "DKT_" #name
#else
#define DKT_ENV_NAME_VARIANT(name) nullptr
#endif
constexpr const char* const DKT_ENV_NAMES[DKT_SW_COUNT] = {
#define X(name, cls) DKT_ENV_NAME_##cls(name),
#include "dkt_switches.def"
#undef X
};

struct DktEnvSnapshot {
    bool set[DKT_SW_COUNT];
    char text[DKT_SW_COUNT][DKT_ENV_VALUE_MAX + 1];
    unsigned generation;                 // + 1 per snapshot; never 0 once one was taken (what was pushed to the device compares it: lds_stage_env_sync, dkt_split.h)
};

DKT_ENV_FN void dkt_env_take(DktEnvSnapshot& e) {
    for (int i = 0; i < DKT_SW_COUNT; ++i) {
        const char* v = DKT_ENV_NAMES[i] ? getenv(DKT_ENV_NAMES[i]) : nullptr;
        e.set[i] = v != nullptr;
        snprintf(e.text[i], sizeof e.text[i], "%s", v ? v : "");
    }
    ++e.generation;
}

DKT_ENV_FN DktEnvSnapshot& dkt_env_snapshot() {
    static DktEnvSnapshot e = [] { DktEnvSnapshot x{}; dkt_env_take(x); return x; }();
    return e;
}
DKT_ENV_FN void dkt_env_reload() { dkt_env_take(dkt_env_snapshot()); }
DKT_ENV_FN unsigned dkt_env_generation() { return dkt_env_snapshot().generation; }

// The snapshotted value, or nullptr when the switch is unset.  A VARIANT switch outside a twins build: always nullptr, a compile-time constant at every call site
// (the compiler drops the variant branches from the product).
DKT_ENV_FN const char* dkt_env(DktSwitch s) {
    if (!DKT_ENV_NAMES[s]) return nullptr;
    const DktEnvSnapshot& e = dkt_env_snapshot();
    return e.set[s] ? e.text[s] : nullptr;
}

// dkt_env_value() / dkt_x16_env_value() of the ABI headers: by name without the DKT_ prefix; nullptr for a name this build does not read.
DKT_ENV_FN const char* dkt_env_by_name(const char* name) {
    for (int i = 0; name && i < DKT_SW_COUNT; ++i)
        if (DKT_ENV_NAMES[i] && !strcmp(DKT_ENV_NAMES[i] + 4, name)) return dkt_env((DktSwitch)i);
    return nullptr;
}

// The three interpretations the call sites use.
DKT_ENV_FN bool dkt_env_on(DktSwitch s) { const char* v = dkt_env(s); return !(v && v[0] == '0'); }               // on unless the value starts with '0'
DKT_ENV_FN bool dkt_env_is(DktSwitch s, char c) { const char* v = dkt_env(s); return v && v[0] == c; }            // set, and the value starts with c
DKT_ENV_FN int dkt_env_int(DktSwitch s, int dflt) { const char* v = dkt_env(s); return v ? atoi(v) : dflt; }      // atoi, or dflt when unset
