// Environment readers for the host-side A/B knobs.  Plain C++, no HIP: tests/native/env_readers_test.cpp
// compiles them alone.  Uncached: a call site that wants the value fixed for the process keeps it in
// a function-local `static const`.  Unset and empty are the same everywhere.
#pragma once
#include <cstdlib>
#include <cstring>

namespace ffc {

inline const char* env_raw(const char* name) {
    const char* e = std::getenv(name);
    return e && *e ? e : nullptr;
}
// atoi of the value (leading integer, 0 for text without one); dflt when unset or empty
inline int env_int(const char* name, int dflt) {
    const char* e = env_raw(name);
    return e ? std::atoi(e) : dflt;
}
// first character of the value; 0 when unset or empty
inline char env_first(const char* name) {
    const char* e = env_raw(name);
    return e ? e[0] : '\0';
}
// the value is exactly `word`
inline bool env_is(const char* name, const char* word) {
    const char* e = env_raw(name);
    return e && std::strcmp(e, word) == 0;
}

}  // namespace ffc
