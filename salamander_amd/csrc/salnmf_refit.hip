// Host side of the refit to fixed signatures (include/salnmf.h: salnmf_refit_exposures) and its two kernels
// (salnmf_refit.h: refit_kernel, refit_reduce_kernel); and of the sparse assignment built on it
// (salnmf_assign_signatures, salnmf_assign_signatures_ex; salnmf_assign.h: assign_kernel, assign_selection_kernel), DESIGN.md sections 14
// and 14.1; and of the goodness-of-fit test built on it (salnmf_draw_model_counts, salnmf_goodness_of_fit; salnmf_gof.h:
// model_draw_kernel, gof_reduce_kernel, which salnmf_batch.hip compiles); and of the signature-presence test
// (salnmf_signature_presence; salnmf_presence.h: presence_kernel here, presence_draw_kernel in salnmf_batch.hip), DESIGN.md section 17;
// and of that test's power analysis (salnmf_signature_power; salnmf_power.h: its three kernels in salnmf_batch.hip), DESIGN.md section 18;
// and of the profile likelihood of one exposure and its interval (salnmf_profile_likelihood, salnmf_exposure_intervals;
// salnmf_profile.h: profile_kernel), DESIGN.md section 19.
#define SALNMF_TEMPLATES_ONLY 1
#define SALNMF_REFIT_KERNELS 1
#include "../../include/salnmf.h"
#include "salnmf_kernels.h"
#include "salnmf_device.h"
#include "salnmf_refit.h"
#include "salnmf_assign.h"
#include "salnmf_gof.h"
#include "salnmf_presence.h"
#include "salnmf_power.h"
#include "salnmf_profile.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

using namespace salnmf;

namespace {

// What both entry points check and prepare before any launch: the ranges, the signatures, the counts clipped to EPSILON
// (and as integers for the resampler when R > 0), the quantiles' indices, the device and its CU count.
struct RefitInputs {
    std::vector<double> x;
    std::vector<uint32_t> icounts;
    std::vector<uint32_t> cand, req;  // the assignment's sets as [N][words] bit masks; empty where the argument is null
    RefitReduceArgs red{};
    int cus = 0;
};

// The assignment's optional sets: one byte per (sample, signature), anything but 0 is "set".
struct AssignSets {
    const uint8_t* candidates = nullptr;
    const uint8_t* required = nullptr;
    int readd = 0;
};

int refit_prepare(int device, const double* counts, int64_t N, int V, const double* signatures, int K, int R, int Q, const double* quantiles,
                  int min_iterations, int max_iterations, int conv_test_freq, double tol, bool resample_outputs, RefitInputs& in,
                  const AssignSets& sets = AssignSets{}) {
    if (N < 1 || N > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)N);
    if (V < 1 || V > VMAX) return fail("n_features must be in [1, %d], got %d", VMAX, V);
    if (K < 1 || K > REFIT_KMAX) return fail("n_signatures must be in [1, %d], got %d", REFIT_KMAX, K);
    if (R < 0 || R > REFIT_SORT_MAX) return fail("n_resamples must be in [0, %d], got %d", REFIT_SORT_MAX, R);
    if (min_iterations < 0 || max_iterations < min_iterations) return fail("need 0 <= min_iterations <= max_iterations, got %d and %d", min_iterations, max_iterations);
    if (conv_test_freq < 1) return fail("conv_test_freq must be positive, got %d", conv_test_freq);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail("tol must be finite and not negative, got %g", tol);
    if (Q < 0 || Q > REFIT_MAX_QUANTILES) return fail("n_quantiles must be in [0, %d], got %d", REFIT_MAX_QUANTILES, Q);
    if (R > 0 && !resample_outputs) return fail("null output for the resamples");
    if (sets.readd != 0 && sets.readd != 1) return fail("readd must be 0 or 1, got %d", sets.readd);
    const int words = ((K + 15) / 16 + 1) / 2;  // assign_kernel<KT>: NW
    auto pack = [&](const uint8_t* set, std::vector<uint32_t>& out) {
        out.assign((size_t)N * words, 0u);
        for (int64_t n = 0; n < N; ++n)
            for (int k = 0; k < K; ++k)
                if (set[(size_t)n * K + k]) out[(size_t)n * words + (k >> 5)] |= 1u << (k & 31);
    };
    if (sets.candidates) {
        pack(sets.candidates, in.cand);
        for (int64_t n = 0; n < N; ++n) {
            uint32_t any = 0u;
            for (int w = 0; w < words; ++w) any |= in.cand[(size_t)n * words + w];
            if (!any) return fail("sample %lld has no candidate signature", (long long)n);
        }
    }
    if (sets.required) {
        pack(sets.required, in.req);
        if (sets.candidates)
            for (size_t i = 0; i < in.req.size(); ++i)
                if (in.req[i] & ~in.cand[i]) {
                    const uint32_t off = in.req[i] & ~in.cand[i];
                    return fail("sample %lld: required signature %d is not a candidate", (long long)(i / words), 32 * (int)(i % words) + __builtin_ctz(off));
                }
    }
    for (int k = 0; k < K; ++k) {
        double sum = 0.0;
        for (int v = 0; v < V; ++v) {
            const double w = signatures[(size_t)k * V + v];
            if (!std::isfinite(w) || w < 0.0) return fail("signature %d, feature %d: entries must be finite and not negative, got %g", k, v, w);
            sum += w;
        }
        if (!(sum > 0.0) || !std::isfinite(sum)) return fail("signature %d needs a positive finite sum", k);
    }
    std::vector<double>& x = in.x;
    x.resize((size_t)N * V);
    for (size_t i = 0; i < x.size(); ++i) {
        if (!std::isfinite(counts[i]) || counts[i] < 0.0)
            return fail("counts must be finite and not negative: row %lld, column %d holds %g", (long long)(i / V), (int)(i % V), counts[i]);
        x[i] = counts[i] < SALNMF_EPSILON ? SALNMF_EPSILON : counts[i];
    }
    if (R > 0) {
        CK(refit_check_counts(counts, N, V, in.icounts));
        for (int i = 0; i < Q; ++i) {
            const double qv = quantiles[i];
            if (!(qv >= 0.0 && qv <= 1.0)) return fail("quantile %d must be in [0, 1], got %g", i, qv);
            // an order statistic, taken outward
            const double pos = qv * (double)(R - 1);
            in.red.index[i] = std::min(R - 1, std::max(0, (int)(qv <= 0.5 ? std::floor(pos) : std::ceil(pos))));
        }
    }
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    in.cus = prop.multiProcessorCount;
    return 0;
}

int launch_refit(const RefitArgs& a, int cus, hipStream_t stream) {
    const int64_t ntiles = (a.P + 15) / 16;
    // one workgroup per CU (the kernel's registers leave room for one wave per SIMD); waves fetch tiles until the list is empty
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)cus, (ntiles + WAVES - 1) / WAVES));
    HIPCK(hipMemsetAsync(a.next_tile, 0, sizeof(unsigned), stream));
    switch ((a.K + 15) / 16) {
        case 1: hipLaunchKernelGGL(refit_kernel<1>, grid, dim3(BLOCK), 0, stream, a); break;
        case 2: hipLaunchKernelGGL(refit_kernel<2>, grid, dim3(BLOCK), 0, stream, a); break;
        case 3: hipLaunchKernelGGL(refit_kernel<3>, grid, dim3(BLOCK), 0, stream, a); break;
        case 4: hipLaunchKernelGGL(refit_kernel<4>, grid, dim3(BLOCK), 0, stream, a); break;
        case 5: hipLaunchKernelGGL(refit_kernel<5>, grid, dim3(BLOCK), 0, stream, a); break;
        case 6: hipLaunchKernelGGL(refit_kernel<6>, grid, dim3(BLOCK), 0, stream, a); break;
        default: return fail("no refit kernel for %d signatures", a.K);
    }
    HIPCK(hipGetLastError());
    return 0;
}

int launch_assign(const AssignArgs& a, int cus, hipStream_t stream) {
    const int64_t ntiles = (a.P + 15) / 16;
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)cus, (ntiles + WAVES - 1) / WAVES));  // as launch_refit
    HIPCK(hipMemsetAsync(a.next_tile, 0, sizeof(unsigned), stream));
    // candidate sets, required signatures and the re-addition pass have instantiations of their own
    const int kt = (a.K + 15) / 16 + (a.cand || a.req || a.readd ? 8 : 0);
    switch (kt) {
        case 1: hipLaunchKernelGGL((assign_kernel<1, false>), grid, dim3(BLOCK), 0, stream, a); break;
        case 2: hipLaunchKernelGGL((assign_kernel<2, false>), grid, dim3(BLOCK), 0, stream, a); break;
        case 3: hipLaunchKernelGGL((assign_kernel<3, false>), grid, dim3(BLOCK), 0, stream, a); break;
        case 4: hipLaunchKernelGGL((assign_kernel<4, false>), grid, dim3(BLOCK), 0, stream, a); break;
        case 5: hipLaunchKernelGGL((assign_kernel<5, false>), grid, dim3(BLOCK), 0, stream, a); break;
        case 6: hipLaunchKernelGGL((assign_kernel<6, false>), grid, dim3(BLOCK), 0, stream, a); break;
        case 9: hipLaunchKernelGGL((assign_kernel<1, true>), grid, dim3(BLOCK), 0, stream, a); break;
        case 10: hipLaunchKernelGGL((assign_kernel<2, true>), grid, dim3(BLOCK), 0, stream, a); break;
        case 11: hipLaunchKernelGGL((assign_kernel<3, true>), grid, dim3(BLOCK), 0, stream, a); break;
        case 12: hipLaunchKernelGGL((assign_kernel<4, true>), grid, dim3(BLOCK), 0, stream, a); break;
        case 13: hipLaunchKernelGGL((assign_kernel<5, true>), grid, dim3(BLOCK), 0, stream, a); break;
        case 14: hipLaunchKernelGGL((assign_kernel<6, true>), grid, dim3(BLOCK), 0, stream, a); break;
        default: return fail("no assignment kernel for %d signatures", a.K);
    }
    HIPCK(hipGetLastError());
    return 0;
}

int launch_presence(const PresenceArgs& a, int cus, hipStream_t stream) {
    const int64_t ntiles = (a.P + 15) / 16;
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)cus, (ntiles + WAVES - 1) / WAVES));  // as launch_refit
    HIPCK(hipMemsetAsync(a.next_tile, 0, sizeof(unsigned), stream));
    switch ((a.K + 15) / 16) {
        case 1: hipLaunchKernelGGL(presence_kernel<1>, grid, dim3(BLOCK), 0, stream, a); break;
        case 2: hipLaunchKernelGGL(presence_kernel<2>, grid, dim3(BLOCK), 0, stream, a); break;
        case 3: hipLaunchKernelGGL(presence_kernel<3>, grid, dim3(BLOCK), 0, stream, a); break;
        case 4: hipLaunchKernelGGL(presence_kernel<4>, grid, dim3(BLOCK), 0, stream, a); break;
        case 5: hipLaunchKernelGGL(presence_kernel<5>, grid, dim3(BLOCK), 0, stream, a); break;
        case 6: hipLaunchKernelGGL(presence_kernel<6>, grid, dim3(BLOCK), 0, stream, a); break;
        default: return fail("no presence kernel for %d signatures", a.K);
    }
    HIPCK(hipGetLastError());
    return 0;
}

int launch_profile(const ProfileArgs& a, int cus, hipStream_t stream) {
    const int64_t ntiles = (a.P + 15) / 16;
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)cus, (ntiles + WAVES - 1) / WAVES));  // as launch_refit
    HIPCK(hipMemsetAsync(a.next_tile, 0, sizeof(unsigned), stream));
    switch ((a.K + 15) / 16) {
        case 1: hipLaunchKernelGGL(profile_kernel<1>, grid, dim3(BLOCK), 0, stream, a); break;
        case 2: hipLaunchKernelGGL(profile_kernel<2>, grid, dim3(BLOCK), 0, stream, a); break;
        case 3: hipLaunchKernelGGL(profile_kernel<3>, grid, dim3(BLOCK), 0, stream, a); break;
        case 4: hipLaunchKernelGGL(profile_kernel<4>, grid, dim3(BLOCK), 0, stream, a); break;
        case 5: hipLaunchKernelGGL(profile_kernel<5>, grid, dim3(BLOCK), 0, stream, a); break;
        case 6: hipLaunchKernelGGL(profile_kernel<6>, grid, dim3(BLOCK), 0, stream, a); break;
        default: return fail("no profile kernel for %d signatures", a.K);
    }
    HIPCK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int salnmf_refit_exposures(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                      int n_resamples, uint64_t seed, int n_quantiles, const double* quantiles, int min_iterations, int max_iterations,
                                      int conv_test_freq, double tol, int64_t chunk_bytes, double* exposures, double* errors, int* n_iterations, int* converged,
                                      double* exposures_quantiles, double* exposures_mean, int* n_iterations_resampled, double* errors_resampled,
                                      double* exposures_resampled, double* timings) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, R = n_resamples, Q = n_quantiles;
    if (!counts || !signatures || !exposures || !errors || !n_iterations || !converged) return fail("null argument");
    RefitInputs in;
    CK(refit_prepare(device, counts, N, V, signatures, K, R, Q, quantiles, min_iterations, max_iterations, conv_test_freq, tol,
                     exposures_mean && n_iterations_resampled && errors_resampled && (Q <= 0 || (quantiles && exposures_quantiles)), in));
    const std::vector<double>& x = in.x;
    const std::vector<uint32_t>& icounts = in.icounts;
    RefitReduceArgs& red = in.red;
    const int cus = in.cus;

    // resamples per chunk: the [chunk][N][V] buffer stays within chunk_bytes (at least one resample)
    const int64_t budget = chunk_bytes > 0 ? chunk_bytes : (int64_t)256 << 20;
    const int chunk = R > 0 ? (int)std::max<int64_t>(1, std::min<int64_t>(R, budget / (int64_t)(sizeof(double) * (size_t)N * V))) : 0;

    // (host buffers of the asynchronous copies live until d's destructor has waited for the stream)
    DevBufs d;
    CK(d.own_stream());
    const size_t NR = (size_t)N * (size_t)std::max(R, 1);
    double* dW = d.get<double>((size_t)K * V);
    double* dX = d.get<double>((size_t)N * V);
    double* dH = d.get<double>((size_t)N * K);
    double* derr = d.get<double>((size_t)N);
    int* dnit = d.get<int>((size_t)N);
    int* dconv = d.get<int>((size_t)N);
    unsigned* dnext = d.get<unsigned>(1);
    if (!dW || !dX || !dH || !derr || !dnit || !dconv || !dnext) return fail("hipMalloc failed (refit of %lld samples)", (long long)N);
    uint32_t* dcounts = nullptr;
    double *dXr = nullptr, *dHr = nullptr, *derr_r = nullptr, *dquant = nullptr, *dmean = nullptr;
    int *dnit_r = nullptr, *dconv_r = nullptr;
    if (R > 0) {
        dcounts = d.get<uint32_t>(icounts.size());
        dXr = d.get<double>((size_t)chunk * N * V);
        dHr = d.get<double>(NR * K);
        derr_r = d.get<double>(NR);
        dnit_r = d.get<int>(NR);
        dconv_r = d.get<int>(NR);
        dquant = d.get<double>((size_t)std::max(Q, 1) * N * K);
        dmean = d.get<double>((size_t)N * K);
        if (!dcounts || !dXr || !dHr || !derr_r || !dnit_r || !dconv_r || !dquant || !dmean)
            return fail("hipMalloc failed (%d resamples of %lld x %d, %d signatures)", R, (long long)N, V, K);
        HIPCK(hipMemcpyAsync(dcounts, icounts.data(), icounts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    }
    HIPCK(hipMemcpyAsync(dW, signatures, (size_t)K * V * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dX, x.data(), x.size() * sizeof(double), hipMemcpyHostToDevice, d.stream));

    RefitArgs a{dX, dW, dH, derr, dnit, dconv, dnext, N, V, K, min_iterations, max_iterations, conv_test_freq, tol};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> t_refit, t_resample, t_reduce;
    auto timed = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>>& into, auto&& body) -> int {
        hipEvent_t e0 = timings ? d.mark() : nullptr;
        CK(body());
        hipEvent_t e1 = timings ? d.mark() : nullptr;
        if (timings && (!e0 || !e1)) return fail("event record failed");
        if (timings) into.emplace_back(e0, e1);
        return 0;
    };
    CK(timed(t_refit, [&] { return launch_refit(a, cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < R; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, R - first);
        CK(timed(t_resample, [&]() -> int {
            refit_launch_resample(dcounts, dXr, N, V, seed, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        RefitArgs c = a;
        c.X = dXr;
        c.P = (int64_t)count * N;
        c.H = dHr + (size_t)first * N * K;
        c.err = derr_r + (size_t)first * N;
        c.nit = dnit_r + (size_t)first * N;
        c.conv = dconv_r + (size_t)first * N;
        CK(timed(t_refit, [&] { return launch_refit(c, cus, d.stream); }));
    }
    if (R > 0) {
        red.H = dHr;
        red.quant = dquant;
        red.mean = dmean;
        red.N = N;
        red.K = K;
        red.R = R;
        red.Q = Q;
        red.R2 = 1;
        while (red.R2 < R) red.R2 <<= 1;
        CK(timed(t_reduce, [&]() -> int {
            hipLaunchKernelGGL(refit_reduce_kernel, dim3((unsigned)N), dim3(REFIT_SORT_BLOCK), 0, d.stream, red);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (Q > 0) HIPCK(hipMemcpyAsync(exposures_quantiles, dquant, (size_t)Q * N * K * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        HIPCK(hipMemcpyAsync(exposures_mean, dmean, (size_t)N * K * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        HIPCK(hipMemcpyAsync(n_iterations_resampled, dnit_r, NR * sizeof(int), hipMemcpyDeviceToHost, d.stream));
        HIPCK(hipMemcpyAsync(errors_resampled, derr_r, NR * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        if (exposures_resampled) HIPCK(hipMemcpyAsync(exposures_resampled, dHr, NR * K * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    }
    HIPCK(hipMemcpyAsync(exposures, dH, (size_t)N * K * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(errors, derr, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(n_iterations, dnit, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(converged, dconv, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipStreamSynchronize(d.stream));
    if (timings) {
        const std::vector<std::pair<hipEvent_t, hipEvent_t>>* sets[3] = {&t_resample, &t_refit, &t_reduce};
        for (int i = 0; i < 3; ++i) {
            double total = 0.0;
            for (const auto& pr : *sets[i]) {
                float ms = 0.f;
                HIPCK(hipEventElapsedTime(&ms, pr.first, pr.second));
                total += (double)ms;
            }
            timings[i] = total;
        }
        timings[3] = (double)n_chunks;
    }
    return 0;
}

extern "C" int salnmf_assign_signatures(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                        int n_resamples, uint64_t seed, int n_quantiles, const double* quantiles, int min_iterations, int max_iterations,
                                        int conv_test_freq, double tol, double max_kl_increase, int64_t chunk_bytes, double* exposures, int* active,
                                        double* errors, int* removal_round, double* kl_increase, int* n_trials, int64_t* n_iterations, int* converged,
                                        double* dense_exposures, double* dense_errors, int* dense_n_iterations, int* dense_converged,
                                        double* selection_frequency, double* exposures_quantiles, double* exposures_mean, double* exposures_resampled,
                                        double* timings) {
    return salnmf_assign_signatures_ex(device, counts, n_samples, n_features, signatures, n_signatures, n_resamples, seed, n_quantiles, quantiles,
                                       min_iterations, max_iterations, conv_test_freq, tol, max_kl_increase, chunk_bytes, nullptr, nullptr, 0, exposures,
                                       active, errors, removal_round, kl_increase, n_trials, n_iterations, converged, dense_exposures, dense_errors,
                                       dense_n_iterations, dense_converged, selection_frequency, exposures_quantiles, exposures_mean, exposures_resampled,
                                       nullptr, nullptr, timings);
}

extern "C" int salnmf_assign_signatures_ex(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                           int n_resamples, uint64_t seed, int n_quantiles, const double* quantiles, int min_iterations,
                                           int max_iterations, int conv_test_freq, double tol, double max_kl_increase, int64_t chunk_bytes,
                                           const uint8_t* candidates, const uint8_t* required, int readd, double* exposures, int* active, double* errors,
                                           int* removal_round, double* kl_increase, int* n_trials, int64_t* n_iterations, int* converged,
                                           double* dense_exposures, double* dense_errors, int* dense_n_iterations, int* dense_converged,
                                           double* selection_frequency, double* exposures_quantiles, double* exposures_mean,
                                           double* exposures_resampled, int* readd_round, double* kl_decrease, double* timings) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, R = n_resamples, Q = n_quantiles;
    if (!counts || !signatures || !exposures || !active || !errors || !removal_round || !kl_increase || !n_trials || !n_iterations || !converged ||
        !dense_exposures || !dense_errors || !dense_n_iterations || !dense_converged)
        return fail("null argument");
    if (readd == 1 && (!readd_round || !kl_decrease)) return fail("null output for the re-addition pass");
    if (!std::isfinite(max_kl_increase)) return fail("max_kl_increase must be finite, got %g", max_kl_increase);
    // (solves follow one another inside one wave, and the tests of its 16 problems must fall on the same iterations)
    if (conv_test_freq >= 1 && max_iterations >= 0 && max_iterations % conv_test_freq != 0)
        return fail("max_iterations must be a multiple of conv_test_freq, got %d and %d", max_iterations, conv_test_freq);
    RefitInputs in;
    CK(refit_prepare(device, counts, N, V, signatures, K, R, Q, quantiles, min_iterations, max_iterations, conv_test_freq, tol,
                     selection_frequency && exposures_mean && (Q <= 0 || (quantiles && exposures_quantiles)), in, AssignSets{candidates, required, readd}));
    const int cus = in.cus;
    const int64_t budget = chunk_bytes > 0 ? chunk_bytes : (int64_t)256 << 20;
    const int chunk = R > 0 ? (int)std::max<int64_t>(1, std::min<int64_t>(R, budget / (int64_t)(sizeof(double) * (size_t)N * V))) : 0;

    DevBufs d;
    CK(d.own_stream());
    const size_t NK = (size_t)N * K, NR = (size_t)N * (size_t)std::max(R, 1);
    double* dW = d.get<double>((size_t)K * V);
    double* dX = d.get<double>((size_t)N * V);
    double* dH = d.get<double>(NK);
    double* dHd = d.get<double>(NK);
    double* dkl = d.get<double>(NK);
    int* dact = d.get<int>(NK);
    int* dround = d.get<int>(NK);
    double* derr = d.get<double>((size_t)N);
    double* derr_d = d.get<double>((size_t)N);
    long long* dnit = d.get<long long>((size_t)N);
    int* dconv = d.get<int>((size_t)N);
    int* dntr = d.get<int>((size_t)N);
    int* dnit_d = d.get<int>((size_t)N);
    int* dconv_d = d.get<int>((size_t)N);
    unsigned* dnext = d.get<unsigned>(1);
    if (!dW || !dX || !dH || !dHd || !dkl || !dact || !dround || !derr || !derr_d || !dnit || !dconv || !dntr || !dnit_d || !dconv_d || !dnext)
        return fail("hipMalloc failed (assignment of %lld samples)", (long long)N);
    uint32_t *dcand = nullptr, *dreq = nullptr;
    int* drround = nullptr;
    double* dkld = nullptr;
    if (candidates) dcand = d.get<uint32_t>(in.cand.size());
    if (required) dreq = d.get<uint32_t>(in.req.size());
    if (readd) drround = d.get<int>(NK), dkld = d.get<double>(NK);
    if ((candidates && !dcand) || (required && !dreq) || (readd && (!drround || !dkld))) return fail("hipMalloc failed (sets of %lld samples)", (long long)N);
    if (dcand) HIPCK(hipMemcpyAsync(dcand, in.cand.data(), in.cand.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    if (dreq) HIPCK(hipMemcpyAsync(dreq, in.req.data(), in.req.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    uint32_t* dcounts = nullptr;
    double *dXr = nullptr, *dHr = nullptr, *derr_r = nullptr, *dquant = nullptr, *dmean = nullptr, *dfreq = nullptr;
    long long* dnit_r = nullptr;
    int *dconv_r = nullptr, *dntr_r = nullptr;
    if (R > 0) {
        dcounts = d.get<uint32_t>(in.icounts.size());
        dXr = d.get<double>((size_t)chunk * N * V);
        dHr = d.get<double>(NR * K);
        derr_r = d.get<double>(NR);
        dnit_r = d.get<long long>(NR);
        dconv_r = d.get<int>(NR);
        dntr_r = d.get<int>(NR);
        dquant = d.get<double>((size_t)std::max(Q, 1) * NK);
        dmean = d.get<double>(NK);
        dfreq = d.get<double>(NK);
        if (!dcounts || !dXr || !dHr || !derr_r || !dnit_r || !dconv_r || !dntr_r || !dquant || !dmean || !dfreq)
            return fail("hipMalloc failed (%d resamples of %lld x %d, %d signatures)", R, (long long)N, V, K);
        HIPCK(hipMemcpyAsync(dcounts, in.icounts.data(), in.icounts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    }
    HIPCK(hipMemcpyAsync(dW, signatures, (size_t)K * V * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dX, in.x.data(), in.x.size() * sizeof(double), hipMemcpyHostToDevice, d.stream));

    AssignArgs a{dX, dW, dH, derr, dnit, dconv, dntr, dact, dround, dkl, dHd, derr_d, dnit_d, dconv_d, dnext, N, V, K,
                 min_iterations, max_iterations, conv_test_freq, tol, max_kl_increase, dcand, dreq, drround, dkld, N, readd};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans[3];  // resample, assign, reduce
    auto timed = [&](int which, auto&& body) -> int {
        hipEvent_t e0 = timings ? d.mark() : nullptr;
        CK(body());
        hipEvent_t e1 = timings ? d.mark() : nullptr;
        if (timings && (!e0 || !e1)) return fail("event record failed");
        if (timings) spans[which].emplace_back(e0, e1);
        return 0;
    };
    CK(timed(1, [&] { return launch_assign(a, cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < R; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, R - first);
        CK(timed(0, [&]() -> int {
            refit_launch_resample(dcounts, dXr, N, V, seed, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        // a resample's problems keep their exposures only: no per-signature record, no phase-0 copy
        AssignArgs c = a;
        c.X = dXr;
        c.P = (int64_t)count * N;
        c.H = dHr + (size_t)first * NK;
        c.err = derr_r + (size_t)first * N;
        c.nit = dnit_r + (size_t)first * N;
        c.conv = dconv_r + (size_t)first * N;
        c.ntrials = dntr_r + (size_t)first * N;
        c.active = nullptr, c.round = nullptr, c.kl = nullptr, c.rround = nullptr, c.kld = nullptr;
        c.dH = nullptr, c.derr = nullptr, c.dnit = nullptr, c.dconv = nullptr;
        CK(timed(1, [&] { return launch_assign(c, cus, d.stream); }));
    }
    if (R > 0) {
        RefitReduceArgs& red = in.red;
        red.H = dHr;
        red.quant = dquant;
        red.mean = dmean;
        red.N = N;
        red.K = K;
        red.R = R;
        red.Q = Q;
        red.R2 = 1;
        while (red.R2 < R) red.R2 <<= 1;
        const AssignSelectArgs sel{dHr, dfreq, (int64_t)NK, R};
        CK(timed(2, [&]() -> int {
            hipLaunchKernelGGL(refit_reduce_kernel, dim3((unsigned)N), dim3(REFIT_SORT_BLOCK), 0, d.stream, red);
            HIPCK(hipGetLastError());
            hipLaunchKernelGGL(assign_selection_kernel, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, d.stream, sel);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (Q > 0) HIPCK(hipMemcpyAsync(exposures_quantiles, dquant, (size_t)Q * NK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        HIPCK(hipMemcpyAsync(exposures_mean, dmean, NK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        HIPCK(hipMemcpyAsync(selection_frequency, dfreq, NK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        if (exposures_resampled) HIPCK(hipMemcpyAsync(exposures_resampled, dHr, NR * K * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    }
    HIPCK(hipMemcpyAsync(exposures, dH, NK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(active, dact, NK * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(removal_round, dround, NK * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(kl_increase, dkl, NK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    if (readd) {
        HIPCK(hipMemcpyAsync(readd_round, drround, NK * sizeof(int), hipMemcpyDeviceToHost, d.stream));
        HIPCK(hipMemcpyAsync(kl_decrease, dkld, NK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    }
    HIPCK(hipMemcpyAsync(errors, derr, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(n_trials, dntr, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(n_iterations, dnit, (size_t)N * sizeof(int64_t), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(converged, dconv, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(dense_exposures, dHd, NK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(dense_errors, derr_d, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(dense_n_iterations, dnit_d, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(dense_converged, dconv_d, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipStreamSynchronize(d.stream));
    if (timings) {
        for (int i = 0; i < 3; ++i) {
            double total = 0.0;
            for (const auto& pr : spans[i]) {
                float ms = 0.f;
                HIPCK(hipEventElapsedTime(&ms, pr.first, pr.second));
                total += (double)ms;
            }
            timings[i] = total;
        }
        timings[3] = (double)n_chunks;
    }
    return 0;
}

// ---- goodness of fit by parametric bootstrap (salnmf_gof.h)

static int gof_check_draws(int n_draws) {
    if (n_draws < 1 || n_draws > GOF_MAX_DRAWS) return fail("n_draws must be in [1, %d], got %d", GOF_MAX_DRAWS, n_draws);
    return 0;
}

extern "C" int salnmf_draw_model_counts(int device, const double* exposures, int64_t n_samples, int n_signatures, const double* signatures,
                                        int n_features, const double* totals, int n_draws, uint64_t seed, double* out) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, B = n_draws;
    if (!exposures || !signatures || !totals || !out) return fail("null argument");
    if (N < 1 || N > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)N);
    if (V < 1 || V > GOF_VMAX) return fail("n_features must be in [1, %d], got %d", GOF_VMAX, V);
    if (K < 1 || K > GOF_KMAX) return fail("n_signatures must be in [1, %d], got %d", GOF_KMAX, K);
    CK(gof_check_draws(B));
    for (size_t i = 0; i < (size_t)N * K; ++i)
        if (!std::isfinite(exposures[i]) || exposures[i] < 0.0)
            return fail("exposures must be finite and not negative: row %lld, signature %d holds %g", (long long)(i / K), (int)(i % K), exposures[i]);
    for (size_t i = 0; i < (size_t)K * V; ++i)
        if (!std::isfinite(signatures[i]) || signatures[i] < 0.0)
            return fail("signature %d, feature %d: entries must be finite and not negative, got %g", (int)(i / V), (int)(i % V), signatures[i]);
    std::vector<uint32_t> trials((size_t)N);
    for (int64_t n = 0; n < N; ++n) {
        const double t = totals[n];
        if (!(t >= 0.0) || t >= 4294967296.0 || t != (double)(uint64_t)t)
            return fail("totals must be non-negative integers below 2^32: row %lld holds %g", (long long)n, t);
        trials[(size_t)n] = (uint32_t)t;
    }
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    const size_t NV = (size_t)N * V;
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)256 << 20) / (int64_t)(sizeof(double) * NV)));
    DevBufs d;
    CK(d.own_stream());
    double* dH = d.get<double>((size_t)N * K);
    double* dW = d.get<double>((size_t)K * V);
    uint32_t* dT = d.get<uint32_t>((size_t)N);
    double* dout = d.get<double>((size_t)chunk * NV);
    if (!dH || !dW || !dT || !dout) return fail("hipMalloc failed (%d draws of %lld x %d)", chunk, (long long)N, V);
    HIPCK(hipMemcpyAsync(dH, exposures, (size_t)N * K * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dW, signatures, (size_t)K * V * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dT, trials.data(), trials.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    for (int first = 0; first < B; first += chunk) {
        const int count = std::min(chunk, B - first);
        gof_launch_model_draw(dH, dW, dT, nullptr, dout, N, V, K, seed, 0.0, first, count, d.stream);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(out + (size_t)first * NV, dout, (size_t)count * NV * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    }
    HIPCK(hipStreamSynchronize(d.stream));
    return 0;
}

extern "C" int salnmf_goodness_of_fit(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                      int n_draws, uint64_t seed, int min_iterations, int max_iterations, int conv_test_freq, double tol,
                                      int64_t chunk_bytes, double* exposures, double* errors, int* n_iterations, int* converged, int* n_exceed,
                                      double* null_mean, double* null_errors, int* null_n_iterations, double* draws, double* timings) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, B = n_draws;
    if (!counts || !signatures || !exposures || !errors || !n_iterations || !converged || !n_exceed || !null_mean || !null_errors || !null_n_iterations)
        return fail("null argument");
    CK(gof_check_draws(B));
    RefitInputs in;
    CK(refit_prepare(device, counts, N, V, signatures, K, 0, 0, nullptr, min_iterations, max_iterations, conv_test_freq, tol, true, in));
    CK(refit_check_counts(counts, N, V, in.icounts));  // integer counts, row totals below 2^32 (the values themselves are not used)
    const int cus = in.cus;
    const size_t NV = (size_t)N * V, NK = (size_t)N * K, NB = (size_t)N * B;

    // draws per chunk: the [chunk][N][V] buffer stays within chunk_bytes (at least one draw)
    const int64_t budget = chunk_bytes > 0 ? chunk_bytes : (int64_t)256 << 20;
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(B, budget / (int64_t)(sizeof(double) * NV)));

    DevBufs d;
    CK(d.own_stream());
    double* dW = d.get<double>((size_t)K * V);
    double* dX = d.get<double>(NV);
    double* dH = d.get<double>(NK);
    double* derr = d.get<double>((size_t)N);
    int* dnit = d.get<int>((size_t)N);
    int* dconv = d.get<int>((size_t)N);
    unsigned* dnext = d.get<unsigned>(1);
    double* dXb = d.get<double>((size_t)chunk * NV);
    double* dHb = d.get<double>((size_t)chunk * NK);
    double* derr_b = d.get<double>(NB);
    int* dnit_b = d.get<int>(NB);
    int* dconv_b = d.get<int>((size_t)chunk * N);
    int* dexceed = d.get<int>((size_t)N);
    double* dmean = d.get<double>((size_t)N);
    if (!dW || !dX || !dH || !derr || !dnit || !dconv || !dnext || !dXb || !dHb || !derr_b || !dnit_b || !dconv_b || !dexceed || !dmean)
        return fail("hipMalloc failed (%d draws of %lld x %d, %d signatures)", B, (long long)N, V, K);
    HIPCK(hipMemcpyAsync(dW, signatures, (size_t)K * V * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dX, in.x.data(), NV * sizeof(double), hipMemcpyHostToDevice, d.stream));

    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans[3];  // draw, refit, reduce
    auto timed = [&](int which, auto&& body) -> int {
        hipEvent_t e0 = timings ? d.mark() : nullptr;
        CK(body());
        hipEvent_t e1 = timings ? d.mark() : nullptr;
        if (timings && (!e0 || !e1)) return fail("event record failed");
        if (timings) spans[which].emplace_back(e0, e1);
        return 0;
    };
    const RefitArgs a{dX, dW, dH, derr, dnit, dconv, dnext, N, V, K, min_iterations, max_iterations, conv_test_freq, tol};
    CK(timed(1, [&] { return launch_refit(a, cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < B; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, B - first);
        // from the device-resident exposures of the observed refit; a row's trial count is read off the clipped counts
        CK(timed(0, [&]() -> int {
            gof_launch_model_draw(dH, dW, nullptr, dX, dXb, N, V, K, seed, SALNMF_EPSILON, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (draws) HIPCK(hipMemcpyAsync(draws + (size_t)first * NV, dXb, (size_t)count * NV * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        RefitArgs c = a;
        c.X = dXb;
        c.P = (int64_t)count * N;
        c.H = dHb;
        c.err = derr_b + (size_t)first * N;
        c.nit = dnit_b + (size_t)first * N;
        c.conv = dconv_b;
        CK(timed(1, [&] { return launch_refit(c, cus, d.stream); }));
    }
    const GofReduceArgs red{derr, derr_b, dexceed, dmean, N, B};
    CK(timed(2, [&]() -> int {
        gof_launch_reduce(red, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    HIPCK(hipMemcpyAsync(exposures, dH, NK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(errors, derr, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(n_iterations, dnit, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(converged, dconv, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(n_exceed, dexceed, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(null_mean, dmean, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(null_errors, derr_b, NB * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(null_n_iterations, dnit_b, NB * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipStreamSynchronize(d.stream));
    if (draws)  // plain counts: the clipped zeros restored to 0
        for (size_t i = 0; i < (size_t)B * NV; ++i)
            if (draws[i] < 1.0) draws[i] = 0.0;
    if (timings) {
        for (int i = 0; i < 3; ++i) {
            double total = 0.0;
            for (const auto& pr : spans[i]) {
                float ms = 0.f;
                HIPCK(hipEventElapsedTime(&ms, pr.first, pr.second));
                total += (double)ms;
            }
            timings[i] = total;
        }
        timings[3] = (double)n_chunks;
    }
    return 0;
}

// ---- is signature s present?  A nested pair of fits against its own bootstrap null (salnmf_presence.h);
// and could the test have seen it?  (salnmf_power.h).  Both entry points run presence_enqueue and
// presence_finish; the power analysis puts its launches on the same stream in between.

namespace {

// salnmf_signature_presence's arguments
struct PresenceIO {
    int device;
    const double* counts;
    int64_t N;
    int V;
    const double* signatures;
    int K;
    const int* test;
    int S;
    const uint8_t* candidates;
    int B;
    uint64_t seed;
    int min_iterations, max_iterations, conv_test_freq;
    double tol;
    int64_t chunk_bytes;
    uint8_t* tested;
    double* statistic;
    int* n_exceed;
    double *null_mean, *exposures, *errors, *null_exposures, *null_errors;
    int *n_iterations, *converged;
    double* null_statistics;
    int* null_n_iterations;
    double *draws, *timings;
};

// What a call keeps between its launches and its results: the pair list, the device buffers and the host ends of the
// asynchronous copies (which live until d's destructor has waited for the stream: d is the last member, and exists once the
// validation has passed and a pair is tested).
struct PresenceRun {
    RefitInputs in;
    std::vector<int> pair_n, pair_s;
    std::vector<size_t> slot;  // pair j is entry slot[j] of the (N, S) results
    std::vector<double> h_stat, h_f, h_H1, h_H0, h_mean, h_stat_b, h_draws;
    std::vector<int> h_nit, h_conv, h_exceed, h_nit_b;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> spans[7];  // draw, solve, reduce; planting, alternative draw, solve, reduce
    size_t NP = 0;
    int64_t chunk_rows = 0;  // rows [pairs][V] of the chunk buffer that chunk_bytes allows
    int n_chunks = 0;
    bool timing = false;
    double *dW = nullptr, *dX = nullptr, *dH0 = nullptr, *dstat_b = nullptr, *dXb = nullptr;
    int *dpn = nullptr, *dps = nullptr;
    PresenceArgs a{};  // the observed launch's
    std::unique_ptr<DevBufs> d;

    template <typename F>
    int timed(int which, F&& body) {
        hipEvent_t e0 = timing ? d->mark() : nullptr;
        CK(body());
        hipEvent_t e1 = timing ? d->mark() : nullptr;
        if (timing && (!e0 || !e1)) return fail("event record failed");
        if (timing) spans[which].emplace_back(e0, e1);
        return 0;
    }
    int span_ms(int which, double* out) {
        double total = 0.0;
        for (const auto& pr : spans[which]) {
            float ms = 0.f;
            HIPCK(hipEventElapsedTime(&ms, pr.first, pr.second));
            total += (double)ms;
        }
        *out = total;
        return 0;
    }
};

int presence_check_test(const int* test, int S, int K) {
    if (S < 1 || S > REFIT_KMAX) return fail("n_test must be in [1, %d], got %d", REFIT_KMAX, S);
    for (int j = 0; j < S; ++j) {
        if (test[j] < 0 || test[j] >= K) return fail("tested signature %d is not in [0, %d)", test[j], K);
        for (int i = 0; i < j; ++i)
            if (test[i] == test[j]) return fail("signature %d is tested twice", test[j]);
    }
    return 0;
}

// The tested pairs, sample after sample: s is a candidate and not the only one.  Pair j is entry slot[j] of the (N, S) results.
void presence_list_pairs(const RefitInputs& in, int64_t N, int K, const int* test, int S, bool with_candidates, uint8_t* tested, std::vector<int>& pair_n,
                         std::vector<int>& pair_s, std::vector<size_t>& slot) {
    const int words = ((K + 15) / 16 + 1) / 2;
    for (int64_t n = 0; n < N; ++n) {
        int size = K;
        if (with_candidates) {
            size = 0;
            for (int w = 0; w < words; ++w) size += __builtin_popcount(in.cand[(size_t)n * words + w]);
        }
        for (int j = 0; j < S; ++j) {
            const int s = test[j];
            const bool member = !with_candidates || ((in.cand[(size_t)n * words + (s >> 5)] >> (s & 31)) & 1u);
            tested[(size_t)n * S + j] = member && size > 1;
            if (member && size > 1) pair_n.push_back((int)n), pair_s.push_back(s), slot.push_back((size_t)n * S + j);
        }
    }
}

// Validation, the pair list, the untested entries of the results, and -- with a tested pair -- everything the presence test puts
// on the stream: the uploads, the observed launch, the null chunks, the reduction and the downloads.  Nothing is waited for.  h0
// (r.dH0, [pairs][K]) and the null statistics (r.dstat_b, [B][pairs]) stay on the device; the chunk buffer r.dXb holds
// min(max(B, other_rows), r.chunk_rows) rows, so that a caller with other_rows draws of its own can reuse it.
int presence_enqueue(const PresenceIO& io, int64_t other_rows, PresenceRun& r) {
    const int64_t N = io.N;
    const int V = io.V, K = io.K, S = io.S, B = io.B;
    const double* counts = io.counts;
    const int* test = io.test;
    const uint8_t* candidates = io.candidates;
    if (!counts || !io.signatures || !test || !io.tested || !io.statistic || !io.n_exceed || !io.null_mean || !io.exposures || !io.errors ||
        !io.null_exposures || !io.null_errors || !io.n_iterations || !io.converged || !io.null_statistics || !io.null_n_iterations)
        return fail("null argument");
    CK(gof_check_draws(B));
    if (io.conv_test_freq >= 1 && io.max_iterations >= 0 && io.max_iterations % io.conv_test_freq != 0)
        return fail("max_iterations must be a multiple of conv_test_freq, got %d and %d", io.max_iterations, io.conv_test_freq);
    CK(presence_check_test(test, S, K));
    RefitInputs& in = r.in;
    CK(refit_prepare(io.device, counts, N, V, io.signatures, K, 0, 0, nullptr, io.min_iterations, io.max_iterations, io.conv_test_freq, io.tol, true, in,
                     AssignSets{candidates, nullptr, 0}));
    CK(refit_check_counts(counts, N, V, in.icounts));  // integer counts, row totals below 2^32 (the values themselves are not used)
    const int cus = in.cus;

    const size_t NS = (size_t)N * S, NV = (size_t)N * V, NK = (size_t)N * K;
    std::vector<int>&pair_n = r.pair_n, &pair_s = r.pair_s;
    presence_list_pairs(in, N, K, test, S, candidates != nullptr, io.tested, pair_n, pair_s, r.slot);
    const size_t NP = pair_n.size();
    if (NP > 0x7fffffff) return fail("%zu tested pairs: at most 2^31 - 1", NP);
    const double nan = std::nan("");
    std::fill(io.statistic, io.statistic + NS, nan);
    std::fill(io.null_mean, io.null_mean + NS, nan);
    std::fill(io.null_errors, io.null_errors + NS, nan);
    std::fill(io.n_exceed, io.n_exceed + NS, 0);
    std::fill(io.exposures, io.exposures + NK, nan);
    std::fill(io.errors, io.errors + N, nan);
    std::fill(io.null_exposures, io.null_exposures + NS * K, nan);
    std::fill(io.n_iterations, io.n_iterations + 2 * NS, 0);
    std::fill(io.converged, io.converged + 2 * NS, 0);
    std::fill(io.null_statistics, io.null_statistics + (size_t)B * NS, nan);
    std::fill(io.null_n_iterations, io.null_n_iterations + 2 * (size_t)B * NS, 0);
    if (io.draws) std::fill(io.draws, io.draws + (size_t)B * NS * V, 0.0);
    if (io.timings) io.timings[0] = io.timings[1] = io.timings[2] = io.timings[3] = 0.0;
    r.NP = NP;
    if (NP == 0) return 0;

    // draws per chunk: the [chunk][pairs][V] buffer stays within chunk_bytes (at least one draw)
    const size_t PV = NP * V, PK = NP * K, PB = NP * B;
    const int64_t budget = io.chunk_bytes > 0 ? io.chunk_bytes : (int64_t)256 << 20;
    r.chunk_rows = std::max<int64_t>(1, budget / (int64_t)(sizeof(double) * PV));
    const int chunk = (int)std::min<int64_t>(B, r.chunk_rows);
    const int64_t buffer_rows = std::min<int64_t>(std::max<int64_t>(B, other_rows), r.chunk_rows);

    r.h_stat.resize(NP), r.h_f.resize(2 * NP), r.h_H1.resize(PK), r.h_H0.resize(PK), r.h_mean.resize(NP), r.h_stat_b.resize(PB);
    r.h_draws.resize(io.draws ? PB * V : 0);
    r.h_nit.resize(2 * NP), r.h_conv.resize(2 * NP), r.h_exceed.resize(NP), r.h_nit_b.resize(2 * PB);
    r.d.reset(new DevBufs);
    DevBufs& d = *r.d;
    CK(d.own_stream());
    double* dW = r.dW = d.get<double>((size_t)K * V);
    double* dX = r.dX = d.get<double>(NV);
    int* dpn = r.dpn = d.get<int>(NP);
    int* dps = r.dps = d.get<int>(NP);
    double* dstat = d.get<double>(NP);
    double* df = d.get<double>(2 * NP);
    int* dnit = d.get<int>(2 * NP);
    int* dconv = d.get<int>(2 * NP);
    double* dH1 = d.get<double>(PK);
    double* dH0 = r.dH0 = d.get<double>(PK);
    unsigned* dnext = d.get<unsigned>(1);
    double* dXb = r.dXb = d.get<double>((size_t)buffer_rows * PV);
    double* dstat_b = r.dstat_b = d.get<double>(PB);
    int* dnit_b = d.get<int>(2 * PB);
    int* dexceed = d.get<int>(NP);
    double* dmean = d.get<double>(NP);
    uint32_t* dcand = candidates ? d.get<uint32_t>(in.cand.size()) : nullptr;
    if (!dW || !dX || !dpn || !dps || !dstat || !df || !dnit || !dconv || !dH1 || !dH0 || !dnext || !dXb || !dstat_b || !dnit_b || !dexceed || !dmean ||
        (candidates && !dcand))
        return fail("hipMalloc failed (%d draws of %zu pairs x %d, %d signatures)", B, NP, V, K);
    HIPCK(hipMemcpyAsync(dW, io.signatures, (size_t)K * V * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dX, in.x.data(), NV * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dpn, pair_n.data(), NP * sizeof(int), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dps, pair_s.data(), NP * sizeof(int), hipMemcpyHostToDevice, d.stream));
    if (dcand) HIPCK(hipMemcpyAsync(dcand, in.cand.data(), in.cand.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));

    r.timing = io.timings != nullptr;
    const PresenceArgs a = r.a = PresenceArgs{dX, dW, dpn, dps, dcand, dstat, dnit, df, dconv, dH1, dH0, dnext, (int64_t)NP, (int64_t)NP, V, K, 1,
                                              io.min_iterations, io.max_iterations, io.conv_test_freq, io.tol};
    CK(r.timed(1, [&] { return launch_presence(a, cus, d.stream); }));
    for (int first = 0; first < B; first += chunk, ++r.n_chunks) {
        const int count = std::min(chunk, B - first);
        // from the device-resident exposures of the observed null fits; a row's trial count is read off the clipped counts
        CK(r.timed(0, [&]() -> int {
            presence_launch_draw(dH0, dW, dX, dpn, dps, dXb, (int64_t)NP, V, K, io.seed, SALNMF_EPSILON, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (io.draws)
            HIPCK(hipMemcpyAsync(r.h_draws.data() + (size_t)first * PV, dXb, (size_t)count * PV * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        // a draw's problems keep their statistic and iteration counts only
        PresenceArgs c = a;
        c.X = dXb;
        c.by_sample = 0;
        c.P = (int64_t)count * (int64_t)NP;
        c.stat = dstat_b + (size_t)first * NP;
        c.nit = dnit_b + 2 * (size_t)first * NP;
        c.f = nullptr, c.conv = nullptr, c.H1 = nullptr, c.H0 = nullptr;
        CK(r.timed(1, [&] { return launch_presence(c, cus, d.stream); }));
    }
    // gof_reduce_kernel over the pairs: n_exceed counts t_b >= t (false for a NaN on either side), null_mean sums from 0.0 in ascending b
    const GofReduceArgs red{dstat, dstat_b, dexceed, dmean, (int64_t)NP, B};
    CK(r.timed(2, [&]() -> int {
        gof_launch_reduce(red, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    HIPCK(hipMemcpyAsync(r.h_stat.data(), dstat, NP * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_f.data(), df, 2 * NP * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_nit.data(), dnit, 2 * NP * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_conv.data(), dconv, 2 * NP * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_H1.data(), dH1, PK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_H0.data(), dH0, PK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_exceed.data(), dexceed, NP * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_mean.data(), dmean, NP * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_stat_b.data(), dstat_b, PB * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_nit_b.data(), dnit_b, 2 * PB * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    return 0;
}

// Waits for the stream, then the compact pair list back into the (N, S) results and the first four timings.
int presence_finish(const PresenceIO& io, PresenceRun& r) {
    const int V = io.V, K = io.K, B = io.B;
    const size_t NP = r.NP, NS = (size_t)io.N * io.S;
    HIPCK(hipStreamSynchronize(r.d->stream));
    // a sample's alternative fit is that of its first tested pair (every tested pair of a sample solves the same problem on C and
    // holds the same bits)
    for (size_t j = 0; j < NP; ++j) {
        const size_t o = r.slot[j], n = (size_t)r.pair_n[j];
        io.statistic[o] = r.h_stat[j];
        io.n_exceed[o] = r.h_exceed[j];
        io.null_mean[o] = r.h_mean[j];
        io.null_errors[o] = r.h_f[2 * j + 1];
        std::copy(r.h_H0.begin() + j * K, r.h_H0.begin() + (j + 1) * K, io.null_exposures + o * K);
        for (int i = 0; i < 2; ++i) io.n_iterations[2 * o + i] = r.h_nit[2 * j + i], io.converged[2 * o + i] = r.h_conv[2 * j + i];
        if (j == 0 || (size_t)r.pair_n[j - 1] != n) {
            std::copy(r.h_H1.begin() + j * K, r.h_H1.begin() + (j + 1) * K, io.exposures + n * K);
            io.errors[n] = r.h_f[2 * j];
        }
        for (size_t b = 0; b < (size_t)B; ++b) {
            io.null_statistics[b * NS + o] = r.h_stat_b[b * NP + j];
            for (int i = 0; i < 2; ++i) io.null_n_iterations[2 * (b * NS + o) + i] = r.h_nit_b[2 * (b * NP + j) + i];
            if (io.draws)  // plain counts: the clipped zeros restored to 0
                for (int v = 0; v < V; ++v) {
                    const double c = r.h_draws[(b * NP + j) * V + v];
                    io.draws[(b * NS + o) * V + v] = c < 1.0 ? 0.0 : c;
                }
        }
    }
    if (io.timings) {
        for (int i = 0; i < 3; ++i) CK(r.span_ms(i, io.timings + i));
        io.timings[3] = (double)r.n_chunks;
    }
    return 0;
}

}  // namespace

extern "C" int salnmf_signature_presence(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                         const int* test, int n_test, const uint8_t* candidates, int n_draws, uint64_t seed, int min_iterations,
                                         int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes, uint8_t* tested, double* statistic,
                                         int* n_exceed, double* null_mean, double* exposures, double* errors, double* null_exposures, double* null_errors,
                                         int* n_iterations, int* converged, double* null_statistics, int* null_n_iterations, double* draws,
                                         double* timings) {
    const PresenceIO io{device, counts, n_samples, n_features, signatures, n_signatures, test, n_test, candidates, n_draws, seed, min_iterations,
                        max_iterations, conv_test_freq, tol, chunk_bytes, tested, statistic, n_exceed, null_mean, exposures, errors, null_exposures,
                        null_errors, n_iterations, converged, null_statistics, null_n_iterations, draws, timings};
    PresenceRun r;
    CK(presence_enqueue(io, 0, r));
    if (r.NP == 0) return 0;
    return presence_finish(io, r);
}

// ---- the presence test's power: the tested signature planted at given shares of the null fit (salnmf_power.h)

extern "C" int salnmf_signature_power(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                      const int* test, int n_test, const uint8_t* candidates, int n_draws, uint64_t seed, int min_iterations,
                                      int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes, const double* shares, int n_shares,
                                      int n_alt_draws, int max_exceed, uint8_t* tested, double* statistic, int* n_exceed, double* null_mean,
                                      double* exposures, double* errors, double* null_exposures, double* null_errors, int* n_iterations, int* converged,
                                      double* null_statistics, int* null_n_iterations, double* draws, double* planted_exposures, double* alt_statistics,
                                      int* alt_n_iterations, int* alt_n_exceed, int* n_detected, double* alt_mean, double* alt_draws, double* timings) {
    const int L = n_shares, A = n_alt_draws, B = n_draws;
    if (!shares || !planted_exposures || !alt_statistics || !alt_n_iterations || !alt_n_exceed || !n_detected || !alt_mean) return fail("null argument");
    CK(gof_check_draws(B));
    if (L < 1 || L > POWER_MAX_SHARES) return fail("n_shares must be in [1, %d], got %d", POWER_MAX_SHARES, L);
    for (int l = 0; l < L; ++l) {
        if (!std::isfinite(shares[l]) || shares[l] < 0.0 || shares[l] >= 1.0) return fail("share %d must be finite and in [0, 1), got %g", l, shares[l]);
        if (l > 0 && !(shares[l] > shares[l - 1])) return fail("shares must be strictly ascending: share %d is %g after %g", l, shares[l], shares[l - 1]);
    }
    if (A < 1 || A > POWER_MAX_DRAWS) return fail("n_alt_draws must be in [1, %d], got %d", POWER_MAX_DRAWS, A);
    if (max_exceed < 0 || max_exceed > B) return fail("max_exceed must be in [0, %d], got %d", B, max_exceed);
    const int64_t R = (int64_t)L * A;  // rows r = l A + a
    const PresenceIO io{device, counts, n_samples, n_features, signatures, n_signatures, test, n_test, candidates, n_draws, seed, min_iterations,
                        max_iterations, conv_test_freq, tol, chunk_bytes, tested, statistic, n_exceed, null_mean, exposures, errors, null_exposures,
                        null_errors, n_iterations, converged, null_statistics, null_n_iterations, draws, timings};
    std::vector<double> h_Hp, h_stat_a, h_mean_a, h_draws_a;  // (before r: they outlive the copies into them, which r.d waits for)
    std::vector<int> h_nit_a, h_exceed_a, h_ndet;
    PresenceRun r;
    CK(presence_enqueue(io, R, r));
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, S = n_test;
    const size_t NS = (size_t)N * S, NP = r.NP;
    const double nan = std::nan("");
    std::fill(planted_exposures, planted_exposures + (size_t)L * NS * K, nan);
    std::fill(alt_statistics, alt_statistics + (size_t)R * NS, nan);
    std::fill(alt_mean, alt_mean + (size_t)L * NS, nan);
    std::fill(alt_n_iterations, alt_n_iterations + 2 * (size_t)R * NS, 0);
    std::fill(alt_n_exceed, alt_n_exceed + (size_t)R * NS, 0);
    std::fill(n_detected, n_detected + (size_t)L * NS, 0);
    if (alt_draws) std::fill(alt_draws, alt_draws + (size_t)R * NS * V, 0.0);
    if (timings) timings[4] = timings[5] = timings[6] = timings[7] = timings[8] = 0.0;
    if (NP == 0) return 0;

    const size_t PV = NP * V, PK = NP * K;
    DevBufs& d = *r.d;
    h_Hp.resize((size_t)L * PK), h_stat_a.resize((size_t)R * NP), h_mean_a.resize((size_t)L * NP), h_draws_a.resize(alt_draws ? (size_t)R * PV : 0);
    h_nit_a.resize(2 * (size_t)R * NP), h_exceed_a.resize((size_t)R * NP), h_ndet.resize((size_t)L * NP);
    double* dshares = d.get<double>((size_t)L);
    double* dHp = d.get<double>((size_t)L * PK);
    double* dstat_a = d.get<double>((size_t)R * NP);
    int* dnit_a = d.get<int>(2 * (size_t)R * NP);
    int* dexceed_a = d.get<int>((size_t)R * NP);
    int* dndet = d.get<int>((size_t)L * NP);
    double* dmean_a = d.get<double>((size_t)L * NP);
    if (!dshares || !dHp || !dstat_a || !dnit_a || !dexceed_a || !dndet || !dmean_a)
        return fail("hipMalloc failed (%d shares x %d draws of %zu pairs x %d, %d signatures)", L, A, NP, V, K);
    HIPCK(hipMemcpyAsync(dshares, shares, (size_t)L * sizeof(double), hipMemcpyHostToDevice, d.stream));
    CK(r.timed(3, [&]() -> int {
        power_launch_plant(PowerPlantArgs{r.dH0, r.dps, dshares, dHp, (int64_t)NP, K, L}, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    // rows per chunk: the presence test's buffer and rule
    const int64_t chunk = std::min<int64_t>(R, r.chunk_rows);
    int n_chunks = 0;
    for (int64_t first = 0; first < R; first += chunk, ++n_chunks) {
        const int64_t count = std::min(chunk, R - first);
        CK(r.timed(4, [&]() -> int {
            power_launch_draw(dHp, r.dW, r.dX, r.dpn, r.dps, r.dXb, (int64_t)NP, V, K, seed, SALNMF_EPSILON, A, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (alt_draws)
            HIPCK(hipMemcpyAsync(h_draws_a.data() + (size_t)first * PV, r.dXb, (size_t)count * PV * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        PresenceArgs c = r.a;  // as a null draw's launch
        c.X = r.dXb;
        c.by_sample = 0;
        c.P = count * (int64_t)NP;
        c.stat = dstat_a + (size_t)first * NP;
        c.nit = dnit_a + 2 * (size_t)first * NP;
        c.f = nullptr, c.conv = nullptr, c.H1 = nullptr, c.H0 = nullptr;
        CK(r.timed(5, [&] { return launch_presence(c, r.in.cus, d.stream); }));
    }
    CK(r.timed(6, [&]() -> int {
        power_launch_reduce(PowerReduceArgs{r.dstat_b, dstat_a, dexceed_a, dndet, dmean_a, (int64_t)NP, B, L, A, max_exceed}, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    HIPCK(hipMemcpyAsync(h_Hp.data(), dHp, h_Hp.size() * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_stat_a.data(), dstat_a, h_stat_a.size() * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_nit_a.data(), dnit_a, h_nit_a.size() * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_exceed_a.data(), dexceed_a, h_exceed_a.size() * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_ndet.data(), dndet, h_ndet.size() * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_mean_a.data(), dmean_a, h_mean_a.size() * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    CK(presence_finish(io, r));  // waits for the stream

    for (size_t j = 0; j < NP; ++j) {
        const size_t o = r.slot[j];
        for (size_t l = 0; l < (size_t)L; ++l) {
            std::copy(h_Hp.begin() + (l * NP + j) * K, h_Hp.begin() + (l * NP + j + 1) * K, planted_exposures + (l * NS + o) * K);
            n_detected[l * NS + o] = h_ndet[l * NP + j];
            alt_mean[l * NS + o] = h_mean_a[l * NP + j];
        }
        for (size_t q = 0; q < (size_t)R; ++q) {
            alt_statistics[q * NS + o] = h_stat_a[q * NP + j];
            alt_n_exceed[q * NS + o] = h_exceed_a[q * NP + j];
            for (int i = 0; i < 2; ++i) alt_n_iterations[2 * (q * NS + o) + i] = h_nit_a[2 * (q * NP + j) + i];
            if (alt_draws)  // plain counts: the clipped zeros restored to 0
                for (int v = 0; v < V; ++v) {
                    const double c = h_draws_a[(q * NP + j) * V + v];
                    alt_draws[(q * NS + o) * V + v] = c < 1.0 ? 0.0 : c;
                }
        }
    }
    if (timings) {
        for (int i = 3; i < 7; ++i) CK(r.span_ms(i, timings + i + 1));
        timings[8] = (double)n_chunks;
    }
    return 0;
}

// ---- the profile likelihood of one exposure and the interval it gives (salnmf_profile.h).  Both entry
// points run profile_observed -- the presence test's observed launch, unchanged -- then list their problems on the host, run one
// profile_kernel launch and scatter its trials.

namespace {

struct ProfileIO {
    int device;
    const double* counts;
    int64_t N;
    int V;
    const double* signatures;
    int K;
    const int* test;
    int S;
    const uint8_t* candidates;
    int min_iterations, max_iterations, conv_test_freq;
    double tol;
    uint8_t* tested;
    double *exposures, *errors;  // the alternative fit: (N, K) and (N)
    double* timings;
};

// The pair list, the observed fits of every pair on the host (stat = f0 - f1, f = (f1, f0), H1) and the device buffers the
// profile launch reads again.  d is the last member: its destructor waits for the stream before the vectors go.
struct ProfileRun {
    RefitInputs in;
    std::vector<int> pair_n, pair_s;
    std::vector<size_t> slot;
    std::vector<double> h_stat, h_f, h_H1;
    size_t NP = 0;
    double *dW = nullptr, *dX = nullptr;
    uint32_t* dcand = nullptr;
    unsigned* dnext = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around the observed launch, around the profile launch
    std::unique_ptr<DevBufs> d;

    int launch(const ProfileIO& io, ProfileArgs a) {
        a.X = dX, a.W = dW, a.cand = dcand, a.next_tile = dnext;
        a.V = io.V, a.K = io.K, a.min_it = io.min_iterations, a.max_it = io.max_iterations, a.freq = io.conv_test_freq, a.tol = io.tol;
        ev[2] = io.timings ? d->mark() : nullptr;
        CK(launch_profile(a, in.cus, d->stream));
        ev[3] = io.timings ? d->mark() : nullptr;
        if (io.timings && (!ev[2] || !ev[3])) return fail("event record failed");
        return 0;
    }
    // (after the stream has been waited for)
    int times(const ProfileIO& io, int64_t P) {
        if (!io.timings) return 0;
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        io.timings[0] = (double)ms;
        HIPCK(hipEventElapsedTime(&ms, ev[2], ev[3]));
        io.timings[1] = (double)ms;
        io.timings[2] = (double)P;
        return 0;
    }
};

// Validation, the pair list, the untested entries of the shared results, and -- with a tested pair -- the observed launch of
// salnmf_signature_presence (the same PresenceArgs: the alternative solve on C, then the null solve, which is the frozen solve
// at 0.0), waited for and copied back.  The counts need not be integers: nothing is drawn.
int profile_observed(const ProfileIO& io, ProfileRun& r) {
    const int64_t N = io.N;
    const int V = io.V, K = io.K, S = io.S;
    if (!io.counts || !io.signatures || !io.test || !io.tested || !io.exposures || !io.errors) return fail("null argument");
    if (io.conv_test_freq >= 1 && io.max_iterations >= 0 && io.max_iterations % io.conv_test_freq != 0)
        return fail("max_iterations must be a multiple of conv_test_freq, got %d and %d", io.max_iterations, io.conv_test_freq);
    CK(presence_check_test(io.test, S, K));
    RefitInputs& in = r.in;
    CK(refit_prepare(io.device, io.counts, N, V, io.signatures, K, 0, 0, nullptr, io.min_iterations, io.max_iterations, io.conv_test_freq, io.tol, true,
                     in, AssignSets{io.candidates, nullptr, 0}));
    presence_list_pairs(in, N, K, io.test, S, io.candidates != nullptr, io.tested, r.pair_n, r.pair_s, r.slot);
    const size_t NP = r.NP = r.pair_n.size();
    if (NP > 0x7fffffff) return fail("%zu tested pairs: at most 2^31 - 1", NP);
    const double nan = std::nan("");
    std::fill(io.exposures, io.exposures + (size_t)N * K, nan);
    std::fill(io.errors, io.errors + N, nan);
    if (io.timings) io.timings[0] = io.timings[1] = io.timings[2] = 0.0;
    if (NP == 0) return 0;

    const size_t PK = NP * K, NV = (size_t)N * V;
    r.h_stat.resize(NP), r.h_f.resize(2 * NP), r.h_H1.resize(PK);
    r.d.reset(new DevBufs);
    DevBufs& d = *r.d;
    CK(d.own_stream());
    double* dW = r.dW = d.get<double>((size_t)K * V);
    double* dX = r.dX = d.get<double>(NV);
    int* dpn = d.get<int>(NP);
    int* dps = d.get<int>(NP);
    double* dstat = d.get<double>(NP);
    double* df = d.get<double>(2 * NP);
    int* dnit = d.get<int>(2 * NP);
    int* dconv = d.get<int>(2 * NP);
    double* dH1 = d.get<double>(PK);
    double* dH0 = d.get<double>(PK);
    unsigned* dnext = r.dnext = d.get<unsigned>(1);
    uint32_t* dcand = r.dcand = io.candidates ? d.get<uint32_t>(in.cand.size()) : nullptr;
    if (!dW || !dX || !dpn || !dps || !dstat || !df || !dnit || !dconv || !dH1 || !dH0 || !dnext || (io.candidates && !dcand))
        return fail("hipMalloc failed (%zu pairs x %d, %d signatures)", NP, V, K);
    HIPCK(hipMemcpyAsync(dW, io.signatures, (size_t)K * V * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dX, in.x.data(), NV * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dpn, r.pair_n.data(), NP * sizeof(int), hipMemcpyHostToDevice, d.stream));
    HIPCK(hipMemcpyAsync(dps, r.pair_s.data(), NP * sizeof(int), hipMemcpyHostToDevice, d.stream));
    if (dcand) HIPCK(hipMemcpyAsync(dcand, in.cand.data(), in.cand.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    const PresenceArgs a{dX, dW, dpn, dps, dcand, dstat, dnit, df, dconv, dH1, dH0, dnext, (int64_t)NP, (int64_t)NP, V, K, 1,
                         io.min_iterations, io.max_iterations, io.conv_test_freq, io.tol};
    r.ev[0] = io.timings ? d.mark() : nullptr;
    CK(launch_presence(a, in.cus, d.stream));
    r.ev[1] = io.timings ? d.mark() : nullptr;
    if (io.timings && (!r.ev[0] || !r.ev[1])) return fail("event record failed");
    HIPCK(hipMemcpyAsync(r.h_stat.data(), dstat, NP * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_f.data(), df, 2 * NP * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(r.h_H1.data(), dH1, PK * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipStreamSynchronize(d.stream));
    // a sample's alternative fit is that of its first tested pair (presence_finish)
    for (size_t j = 0; j < NP; ++j)
        if (j == 0 || r.pair_n[j - 1] != r.pair_n[j]) {
            const size_t n = (size_t)r.pair_n[j];
            std::copy(r.h_H1.begin() + j * K, r.h_H1.begin() + (j + 1) * K, io.exposures + n * K);
            io.errors[n] = r.h_f[2 * j];
        }
    return 0;
}

template <typename T>
T* profile_upload(DevBufs& d, const std::vector<T>& host) {
    T* dev = d.get<T>(host.size());
    if (dev && hipMemcpyAsync(dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, d.stream) != hipSuccess) return nullptr;
    return dev;
}

}  // namespace

extern "C" int salnmf_profile_likelihood(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                         const int* test, int n_test, const uint8_t* candidates, const double* values, int n_values, int values_per_pair,
                                         int min_iterations, int max_iterations, int conv_test_freq, double tol, uint8_t* tested, double* profile,
                                         double* profile_errors, int* n_iterations, int* converged, double* profile_exposures, double* exposures,
                                         double* errors, double* timings) {
    const int64_t N = n_samples;
    const int K = n_signatures, S = n_test, M = n_values;
    if (!values || !profile || !profile_errors || !n_iterations || !converged) return fail("null argument");
    if (M < 1 || M > PROFILE_MAX_VALUES) return fail("n_values must be in [1, %d], got %d", PROFILE_MAX_VALUES, M);
    if (values_per_pair != 0 && values_per_pair != 1) return fail("values_per_pair must be 0 or 1, got %d", values_per_pair);
    if (N < 1 || N > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)N);
    if (S < 1 || S > REFIT_KMAX) return fail("n_test must be in [1, %d], got %d", REFIT_KMAX, S);
    const size_t NS = (size_t)N * S, n_given = values_per_pair ? NS * M : (size_t)M;
    for (size_t i = 0; i < n_given; ++i)
        if (!std::isfinite(values[i]) || values[i] < 0.0) return fail("values must be finite and not negative: entry %zu holds %g", i, values[i]);
    const ProfileIO io{device, counts, N, n_features, signatures, K, test, S, candidates, min_iterations, max_iterations, conv_test_freq, tol, tested,
                       exposures, errors, timings};
    // (before r: they outlive the copies into and out of them, which r.d waits for)
    std::vector<int> prob_n, prob_s, count, h_nit, h_conv;
    std::vector<double> vals, h_f, h_H;
    ProfileRun r;
    CK(profile_observed(io, r));
    const double nan = std::nan("");
    std::fill(profile, profile + NS * M, nan);
    std::fill(profile_errors, profile_errors + NS * M, nan);
    std::fill(n_iterations, n_iterations + NS * M, 0);
    std::fill(converged, converged + NS * M, 0);
    if (profile_exposures) std::fill(profile_exposures, profile_exposures + NS * M * K, nan);
    const size_t NP = r.NP;
    if (NP == 0) return 0;

    // a problem is a pair and one run of its values
    const int T = std::min(M, PROFILE_RUN), runs = (M + T - 1) / T;
    const size_t P = NP * runs;
    if (P > 0x7fffffff) return fail("%zu problems (%zu pairs x %d runs of values): at most 2^31 - 1", P, NP, runs);
    prob_n.resize(P), prob_s.resize(P), count.resize(P), vals.assign(P * T, 0.0);
    for (size_t j = 0; j < NP; ++j)
        for (int run = 0; run < runs; ++run) {
            const size_t p = j * runs + run;
            prob_n[p] = r.pair_n[j], prob_s[p] = r.pair_s[j], count[p] = std::min(T, M - run * T);
            const double* from = values + (values_per_pair ? r.slot[j] * M : 0) + (size_t)run * T;
            std::copy(from, from + count[p], vals.begin() + p * T);
        }
    h_f.resize(P * T), h_nit.resize(P * T), h_conv.resize(P * T), h_H.resize(profile_exposures ? P * T * K : 0);
    DevBufs& d = *r.d;
    ProfileArgs a{};
    a.prob_n = profile_upload(d, prob_n), a.prob_s = profile_upload(d, prob_s), a.count = profile_upload(d, count), a.values = profile_upload(d, vals);
    a.trial_f = d.get<double>(P * T), a.trial_nit = d.get<int>(P * T), a.trial_conv = d.get<int>(P * T);
    a.trial_H = profile_exposures ? d.get<double>(P * T * K) : nullptr;
    if (!a.prob_n || !a.prob_s || !a.count || !a.values || !a.trial_f || !a.trial_nit || !a.trial_conv || (profile_exposures && !a.trial_H))
        return fail("hipMalloc or upload failed (%zu problems of %d values, %d signatures)", P, T, K);
    a.P = (int64_t)P, a.T = T;
    CK(r.launch(io, a));
    HIPCK(hipMemcpyAsync(h_f.data(), a.trial_f, h_f.size() * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_nit.data(), a.trial_nit, h_nit.size() * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_conv.data(), a.trial_conv, h_conv.size() * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    if (a.trial_H) HIPCK(hipMemcpyAsync(h_H.data(), a.trial_H, h_H.size() * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipStreamSynchronize(d.stream));
    for (size_t p = 0; p < P; ++p) {
        const size_t j = p / runs, run = p % runs;
        const double f1 = r.h_f[2 * j];
        for (int i = 0; i < count[p]; ++i) {
            const size_t from = p * T + i, to = r.slot[j] * M + run * T + i;
            profile[to] = h_f[from] - f1;  // one rounded subtraction, as presence_kernel's statistic
            profile_errors[to] = h_f[from], n_iterations[to] = h_nit[from], converged[to] = h_conv[from];
            if (profile_exposures) std::copy(h_H.begin() + from * K, h_H.begin() + (from + 1) * K, profile_exposures + to * K);
        }
    }
    return r.times(io, (int64_t)P);
}

extern "C" int salnmf_exposure_intervals(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                         const int* test, int n_test, const uint8_t* candidates, double max_kl_increase, int n_bisections,
                                         int max_expansions, int min_iterations, int max_iterations, int conv_test_freq, double tol, uint8_t* tested,
                                         double* lower, double* upper, double* estimate, uint8_t* bracketed, int* n_trials, double* statistic,
                                         double* null_errors, double* exposures, double* errors, double* trace_values, double* trace_profile,
                                         double* timings) {
    const int64_t N = n_samples;
    const int K = n_signatures, S = n_test, J = n_bisections, E = max_expansions;
    const double delta = max_kl_increase;
    if (!lower || !upper || !estimate || !bracketed || !n_trials || !statistic || !null_errors || (trace_values == nullptr) != (trace_profile == nullptr))
        return fail("null argument");
    if (!std::isfinite(delta) || delta < 0.0) return fail("max_kl_increase must be finite and not negative, got %g", delta);
    if (J < 0 || J > PROFILE_MAX_BISECTIONS) return fail("n_bisections must be in [0, %d], got %d", PROFILE_MAX_BISECTIONS, J);
    if (E < 1 || E > PROFILE_MAX_EXPANSIONS) return fail("max_expansions must be in [1, %d], got %d", PROFILE_MAX_EXPANSIONS, E);
    if (N < 1 || N > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)N);
    if (S < 1 || S > REFIT_KMAX) return fail("n_test must be in [1, %d], got %d", REFIT_KMAX, S);
    const ProfileIO io{device, counts, N, n_features, signatures, K, test, S, candidates, min_iterations, max_iterations, conv_test_freq, tol, tested,
                       exposures, errors, timings};
    std::vector<int> prob_n, prob_s, end, h_nt, h_br;
    std::vector<double> hhat, f1, h_c, h_f, h_lo, h_hi;
    std::vector<size_t> prob_pair;
    ProfileRun r;
    CK(profile_observed(io, r));
    const int T = E + J;
    const size_t NS = (size_t)N * S, NP = r.NP;
    const double nan = std::nan("");
    for (double* out : {lower, upper, estimate, statistic, null_errors}) std::fill(out, out + NS, nan);
    std::fill(bracketed, bracketed + NS, (uint8_t)0);
    std::fill(n_trials, n_trials + 2 * NS, 0);
    if (trace_values) std::fill(trace_values, trace_values + 2 * NS * T, nan), std::fill(trace_profile, trace_profile + 2 * NS * T, nan);
    if (NP == 0) return 0;

    // a problem is a pair and one end; a lower end with g(0) <= delta is 0.0 without a trial
    for (size_t j = 0; j < NP; ++j) {
        const size_t o = r.slot[j];
        const double hh = r.h_H1[j * K + r.pair_s[j]];
        estimate[o] = hh, statistic[o] = r.h_stat[j], null_errors[o] = r.h_f[2 * j + 1];
        lower[o] = 0.0;
        for (int which = 0; which < 2; ++which) {
            if (which == 0 && r.h_stat[j] <= delta) continue;
            prob_pair.push_back(j), prob_n.push_back(r.pair_n[j]), prob_s.push_back(r.pair_s[j]), end.push_back(which);
            hhat.push_back(hh), f1.push_back(r.h_f[2 * j]);
        }
    }
    const size_t P = prob_pair.size();
    h_c.resize(P * T), h_f.resize(P * T), h_lo.resize(P), h_hi.resize(P), h_nt.resize(P), h_br.resize(P);
    DevBufs& d = *r.d;
    ProfileArgs a{};
    a.prob_n = profile_upload(d, prob_n), a.prob_s = profile_upload(d, prob_s), a.end = profile_upload(d, end);
    a.hhat = profile_upload(d, hhat), a.f1 = profile_upload(d, f1);
    a.trial_c = d.get<double>(P * T), a.trial_f = d.get<double>(P * T), a.trial_nit = d.get<int>(P * T), a.trial_conv = d.get<int>(P * T);
    a.lo = d.get<double>(P), a.hi = d.get<double>(P), a.n_trials = d.get<int>(P), a.bracketed = d.get<int>(P);
    if (!a.prob_n || !a.prob_s || !a.end || !a.hhat || !a.f1 || !a.trial_c || !a.trial_f || !a.trial_nit || !a.trial_conv || !a.lo || !a.hi ||
        !a.n_trials || !a.bracketed)
        return fail("hipMalloc or upload failed (%zu problems of %d trials, %d signatures)", P, T, K);
    a.P = (int64_t)P, a.T = T, a.n_bisections = J, a.max_expansions = E, a.delta = delta;
    CK(r.launch(io, a));
    HIPCK(hipMemcpyAsync(h_c.data(), a.trial_c, h_c.size() * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_f.data(), a.trial_f, h_f.size() * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_lo.data(), a.lo, P * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_hi.data(), a.hi, P * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_nt.data(), a.n_trials, P * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipMemcpyAsync(h_br.data(), a.bracketed, P * sizeof(int), hipMemcpyDeviceToHost, d.stream));
    HIPCK(hipStreamSynchronize(d.stream));
    for (size_t p = 0; p < P; ++p) {
        const size_t o = r.slot[prob_pair[p]];
        const int which = end[p];
        if (which == 0) lower[o] = h_lo[p];
        else upper[o] = h_br[p] ? h_hi[p] : INFINITY, bracketed[o] = h_br[p] != 0;
        n_trials[2 * o + which] = h_nt[p];
        if (trace_values)
            for (int i = 0; i < h_nt[p]; ++i) {
                trace_values[(2 * o + which) * T + i] = h_c[p * T + i];
                trace_profile[(2 * o + which) * T + i] = h_f[p * T + i] - f1[p];  // the kernel's own g, one rounded subtraction
            }
    }
    return r.times(io, (int64_t)P);
}
