// The library's error channel, shared by its translation units: an entry point that fails returns nonzero and leaves its
// message in g_err, one per host thread (include/salnmf.h: salnmf_last_error, salnmf_batch_last_error).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

namespace salnmf {

inline thread_local std::string g_err;

inline int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

}  // namespace salnmf

#define HIPCK(call)                                                                              \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define CK(call)               \
    do {                       \
        int rc_ = (call);      \
        if (rc_) return rc_;   \
    } while (0)
