// ct_env.h -- the one place where libct_hip.so reads its environment (host code only).  Part of ct_common.h; a source that wants
// nothing else of ct_common.h (attention16.hip: ct_common.h would add its zeroing kernel to that code object) includes this file.
#pragma once
#include <cstdio>
#include <cstdlib>

namespace ct {

// ---- start-up switches ------------------------------------------------------------------------------------------------------------
// Every environment switch of the library is read here (host code; the table of switches is in DESIGN.md).  A call site consults
// its switch once, from a function-local static, and keeps its own range check and default.  With CT_HIP_ENV_TRACE=1 each consult
// writes one line to stderr:  ct_hip env NAME=<raw text or (unset)> -> <value handed to the call site>
// (tests/test_kernel_variants_gpu.py: the proof that a child process with a switch set reached the launcher that owns it).
inline bool env_trace() {
    static const bool on = [] { const char *t = getenv("CT_HIP_ENV_TRACE"); return t && atoi(t) != 0; }();
    return on;
}
// the switch as an integer (atoi of its text), `dflt` when it is not set
inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    const int v = e ? atoi(e) : dflt;
    if (env_trace()) fprintf(stderr, "ct_hip env %s=%s -> %d\n", name, e ? e : "(unset)", v);
    return v;
}
// the switch's text, nullptr when it is not set (CT_HIP_LAB and the switches that test their first character)
inline const char *env_str(const char *name) {
    const char *e = getenv(name);
    if (env_trace()) fprintf(stderr, "ct_hip env %s=%s -> %s\n", name, e ? e : "(unset)", e ? e : "(unset)");
    return e;
}

}  // namespace ct
