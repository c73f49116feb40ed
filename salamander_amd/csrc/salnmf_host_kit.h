// The part of the refit family's host kit that holds no kernel: the span timer, the chunk rule and the
// asynchronous copies.  salnmf_refit.hip (the tile launcher and the reduce fill stay there, next to their kernels) and
// salnmf_information.hip write their drivers with it.
#pragma once
#include "salnmf_device.h"

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace salnmf {

// Device-event spans around groups of launches on d's stream, summed per group; nothing is recorded unless `on`.
struct Spans {
    static constexpr int GROUPS = 7;  // the most any driver has (the power analysis)
    DevBufs* d = nullptr;
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans[GROUPS];

    void start(DevBufs& bufs, bool timing) { d = &bufs, on = timing; }
    template <typename F>
    int timed(int which, F&& body) {
        if (which < 0 || which >= GROUPS) return fail("span group %d out of range", which);
        hipEvent_t e0 = on ? d->mark() : nullptr;
        CK(body());
        hipEvent_t e1 = on ? d->mark() : nullptr;
        if (on && (!e0 || !e1)) return fail("event record failed");
        if (on) spans[which].emplace_back(e0, e1);
        return 0;
    }
    // (after the stream has been waited for)
    int total_ms(int which, double* out) {
        double total = 0.0;
        for (const auto& pr : spans[which]) {
            float ms = 0.f;
            HIPCK(hipEventElapsedTime(&ms, pr.first, pr.second));
            total += (double)ms;
        }
        *out = total;
        return 0;
    }
    // groups 0 .. count - 1 into out[0 .. count - 1]; nothing when timing is off
    int totals(int count, double* out) {
        for (int i = 0; on && i < count; ++i) CK(total_ms(i, out + i));
        return 0;
    }
};

// Rows of a chunk buffer: as many of `rows` as budget_bytes allows (0 or less: 256 MiB), at least one
inline int64_t chunk_rows(int64_t budget_bytes, size_t row_bytes, int64_t rows) {
    const int64_t budget = budget_bytes > 0 ? budget_bytes : (int64_t)256 << 20;
    return std::max<int64_t>(1, std::min<int64_t>(rows, budget / (int64_t)row_bytes));
}

// n entries of `host` in a new buffer of d, copied on its stream: the device pointer, or null (the allocation or the copy
// failed).  The host side lives until d's destructor has waited for the stream: it is declared before d.
template <typename T>
T* upload(DevBufs& d, const T* host, size_t n) {
    T* dev = d.get<T>(n);
    if (dev && hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, d.stream) != hipSuccess) return nullptr;
    return dev;
}
template <typename T>
T* upload(DevBufs& d, const std::vector<T>& host) {
    return upload(d, host.data(), host.size());
}

// n entries of the device buffer `src` to `dst` on d's stream (not waited for)
template <typename D, typename S>
int download(DevBufs& d, D* dst, const S* src, size_t n) {
    static_assert(sizeof(D) == sizeof(S), "download: element sizes differ");
    HIPCK(hipMemcpyAsync(dst, src, n * sizeof(S), hipMemcpyDeviceToHost, d.stream));
    return 0;
}
template <typename T, typename S>
int download(DevBufs& d, std::vector<T>& dst, const S* src) {
    return download(d, dst.data(), src, dst.size());
}

}  // namespace salnmf
