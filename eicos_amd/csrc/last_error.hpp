// The calling thread's error message -- what eicos_last_error (api.cpp) returns -- and the one way to set it together with a return code.
// Host only, no HIP: api.cpp, plan_step.cpp and host_check.cpp share this one slot (multi.cpp keeps its own for the eicos_multi calls).
#pragma once

#include <string>

namespace eicos {
#pragma GCC visibility push(hidden) // (internal to the library: not part of its exported symbols)
inline thread_local std::string g_err;
inline int fail(int code, const std::string &msg) { g_err = msg; return code; }
#pragma GCC visibility pop
} // namespace eicos
