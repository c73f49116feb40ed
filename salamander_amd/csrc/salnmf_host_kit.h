// The part of the refit family's host kit that holds no kernel: the span timer, the chunk rule, the
// asynchronous copies, the tile launcher, and the checks that the entry points of salnmf_refit.hip and salnmf_nb.hip make of
// their arguments before they open a device.  salnmf_refit.hip, salnmf_nb.hip and salnmf_information.hip write their drivers
// with it (the first two through salnmf_refit_drivers.h).  Included after salnmf_kernels.h (WAVES, VMAX), as salnmf_refit.h is.
#pragma once
#include "salnmf_device.h"
#include "salnmf_gof.h"
#include "salnmf_refit.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
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

// What every tile-solve kernel's launch does: one workgroup per CU (the kernels' registers leave room for one wave per SIMD; waves
// fetch tiles until the list is empty), the list's head reset, and the instantiation for (K + 15) / 16 signature tiles, which
// `launch` gets as a std::integral_constant.
template <typename Launch>
int launch_tiles(const char* what, int64_t P, int K, unsigned* next_tile, int cus, hipStream_t stream, Launch&& launch) {
    const int64_t ntiles = (P + 15) / 16;
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)cus, (ntiles + WAVES - 1) / WAVES));
    HIPCK(hipMemsetAsync(next_tile, 0, sizeof(unsigned), stream));
    switch ((K + 15) / 16) {
        case 1: launch(std::integral_constant<int, 1>{}, grid); break;
        case 2: launch(std::integral_constant<int, 2>{}, grid); break;
        case 3: launch(std::integral_constant<int, 3>{}, grid); break;
        case 4: launch(std::integral_constant<int, 4>{}, grid); break;
        case 5: launch(std::integral_constant<int, 5>{}, grid); break;
        case 6: launch(std::integral_constant<int, 6>{}, grid); break;
        default: return fail("no %s kernel for %d signatures", what, K);
    }
    HIPCK(hipGetLastError());
    return 0;
}

// ---- what the entry points check on the host, in the order every one of them keeps: the ranges, (the entry point's own: the
// assignment's sets, the dispersions,) the signatures, the counts, the quantiles.  A call with no resamples passes R = Q = 0 and
// resample_outputs = true.

inline int check_refit_ranges(int64_t N, int V, int K, int R, int min_iterations, int max_iterations, int conv_test_freq, double tol, int Q,
                              bool resample_outputs) {
    if (N < 1 || N > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)N);
    if (V < 1 || V > VMAX) return fail("n_features must be in [1, %d], got %d", VMAX, V);
    if (K < 1 || K > REFIT_KMAX) return fail("n_signatures must be in [1, %d], got %d", REFIT_KMAX, K);
    if (R < 0 || R > REFIT_SORT_MAX) return fail("n_resamples must be in [0, %d], got %d", REFIT_SORT_MAX, R);
    if (min_iterations < 0 || max_iterations < min_iterations) return fail("need 0 <= min_iterations <= max_iterations, got %d and %d", min_iterations, max_iterations);
    if (conv_test_freq < 1) return fail("conv_test_freq must be positive, got %d", conv_test_freq);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail("tol must be finite and not negative, got %g", tol);
    if (Q < 0 || Q > REFIT_MAX_QUANTILES) return fail("n_quantiles must be in [0, %d], got %d", REFIT_MAX_QUANTILES, Q);
    if (R > 0 && !resample_outputs) return fail("null output for the resamples");
    return 0;
}

// The signature rows: finite, not negative, each of positive finite sum
inline int check_signatures(const double* signatures, int K, int V) {
    for (int k = 0; k < K; ++k) {
        double sum = 0.0;
        for (int v = 0; v < V; ++v) {
            const double w = signatures[(size_t)k * V + v];
            if (!std::isfinite(w) || w < 0.0) return fail("signature %d, feature %d: entries must be finite and not negative, got %g", k, v, w);
            sum += w;
        }
        if (!(sum > 0.0) || !std::isfinite(sum)) return fail("signature %d needs a positive finite sum", k);
    }
    return 0;
}

// The counts, finite and not negative, as x = max(counts, EPSILON)
inline int clip_counts(const double* counts, int64_t N, int V, std::vector<double>& x) {
    x.resize((size_t)N * V);
    for (size_t i = 0; i < x.size(); ++i) {
        if (!std::isfinite(counts[i]) || counts[i] < 0.0)
            return fail("counts must be finite and not negative: row %lld, column %d holds %g", (long long)(i / V), (int)(i % V), counts[i]);
        x[i] = counts[i] < SALNMF_EPSILON ? SALNMF_EPSILON : counts[i];
    }
    return 0;
}

// What a call with R > 0 resamples needs besides: the counts as integers for the resampler, and every quantile's index into the R
// sorted values (RefitReduceArgs::index) -- an order statistic, taken outward
inline int check_resamples(const double* counts, int64_t N, int V, int R, int Q, const double* quantiles, std::vector<uint32_t>& icounts, int* index) {
    CK(refit_check_counts(counts, N, V, icounts));
    for (int i = 0; i < Q; ++i) {
        const double qv = quantiles[i];
        if (!(qv >= 0.0 && qv <= 1.0)) return fail("quantile %d must be in [0, 1], got %g", i, qv);
        const double pos = qv * (double)(R - 1);
        index[i] = std::min(R - 1, std::max(0, (int)(qv <= 0.5 ? std::floor(pos) : std::ceil(pos))));
    }
    return 0;
}

inline int check_n_draws(int n_draws) {
    if (n_draws < 1 || n_draws > GOF_MAX_DRAWS) return fail("n_draws must be in [1, %d], got %d", GOF_MAX_DRAWS, n_draws);
    return 0;
}

// What both draws from a fitted model (salnmf_draw_model_counts, salnmf_draw_nb_counts) check of the model and the draw count
inline int check_model_draw(const double* exposures, int64_t N, int K, const double* signatures, int V, int B) {
    if (N < 1 || N > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)N);
    if (V < 1 || V > GOF_VMAX) return fail("n_features must be in [1, %d], got %d", GOF_VMAX, V);
    if (K < 1 || K > GOF_KMAX) return fail("n_signatures must be in [1, %d], got %d", GOF_KMAX, K);
    CK(check_n_draws(B));
    for (size_t i = 0; i < (size_t)N * K; ++i)
        if (!std::isfinite(exposures[i]) || exposures[i] < 0.0)
            return fail("exposures must be finite and not negative: row %lld, signature %d holds %g", (long long)(i / K), (int)(i % K), exposures[i]);
    for (size_t i = 0; i < (size_t)K * V; ++i)
        if (!std::isfinite(signatures[i]) || signatures[i] < 0.0)
            return fail("signature %d, feature %d: entries must be finite and not negative, got %g", (int)(i / V), (int)(i % V), signatures[i]);
    return 0;
}

}  // namespace salnmf
