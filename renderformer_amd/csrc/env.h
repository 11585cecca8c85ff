// One way to read an RF_* environment knob (DESIGN.md §3.1 lists every knob of gemm.hip).
//   env_int(name, dflt)       read on every call: tests and A/B tools flip these inside one process
//   RF_ENV_ONCE(name, dflt)   read once per call site (first use) and kept for the life of the process
//   env_str(name)             the raw string of a knob that is not a number (null when unset), read on every call
// An unset variable gives dflt; a set one gives atoi of its value (so "" and "x" read as 0).
#pragma once
#include <stdlib.h>

namespace rf {

inline bool env_set(const char* name) { return getenv(name) != nullptr; }

inline const char* env_str(const char* name) { return getenv(name); }

inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

}  // namespace rf

#define RF_ENV_ONCE(name, dflt)                         \
    ([]() -> int {                                      \
        static const int v = ::rf::env_int(name, dflt); \
        return v;                                       \
    }())
