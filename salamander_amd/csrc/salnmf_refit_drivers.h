// The four host drivers that the Poisson entry points (salnmf_refit.hip: salnmf_refit_exposures, salnmf_goodness_of_fit,
// salnmf_draw_model_counts, salnmf_assign_signatures_ex) and their negative-binomial counterparts (salnmf_nb.hip, and
// salnmf_nb_assign.hip for the assignment) share, DESIGN.md section 13.1.  The two sides differ in the kernel's argument struct
// (RefitArgs, NbRefitArgs; AssignArgs, NbAssignArgs), its launcher and the draw call, so each driver is a
// template over those and an entry point is its checks, the uploads of its model's own inputs and one call.  Host code only:
// no kernel is defined or named here.  A driver issues its launches, memsets and copies in one fixed order on d's stream;
// tests/test_gpu_refit_family_bits.py and tests/test_gpu_nb_family_bits.py hold both sides to the bits that order gives.
// The fifth, the pair run at the end of this file, is what salnmf_signature_presence (with the power analysis and the profile
// calls that start like it) and salnmf_nb_signature_presence (salnmf_nb_presence.hip) share, DESIGN.md sections 17 and 26.
#pragma once
#include "salnmf_host_kit.h"
#include "salnmf_assign.h"
#include "salnmf_nb.h"
#include "salnmf_presence.h"

#include <memory>

namespace salnmf {

// The dispersions of a negative-binomial entry point: one per sample, finite and in (0, NB_ALPHA_MAX]
inline int nb_check_dispersion(const double* dispersion, int64_t N) {
    for (int64_t n = 0; n < N; ++n)
        if (!std::isfinite(dispersion[n]) || !(dispersion[n] > 0.0) || dispersion[n] > NB_ALPHA_MAX)
            return fail("dispersion must be finite and in (0, %g]: sample %lld holds %g", NB_ALPHA_MAX, (long long)n, dispersion[n]);
    return 0;
}

// The gamma draw's per-sample constants (salnmf_nbdraw.h): d = a' - 1/3 and c = 1 / sqrt(9 d), a' = alpha (alpha >= 1) or alpha + 1:
// computed on the host, so that the kernel's gamma path has no square root of its own
inline void nb_gamma_constants(const double* dispersion, int64_t N, std::vector<double>& gd, std::vector<double>& gc) {
    gd.resize((size_t)N), gc.resize((size_t)N);
    for (int64_t n = 0; n < N; ++n) {
        const double shape = dispersion[n] >= 1.0 ? dispersion[n] : dispersion[n] + 1.0;
        gd[(size_t)n] = shape - 1.0 / 3.0;
        gc[(size_t)n] = 1.0 / std::sqrt(9.0 * gd[(size_t)n]);
    }
}

// sum_v sum_k h_k W[k, v] of one exposure row, as the negative-binomial draw's entry points bound it (NB_MAX_MEAN)
inline double nb_model_row_sum(const double* h, const double* signatures, int K, int V) {
    double mean = 0.0;
    for (int v = 0; v < V; ++v)
        for (int k = 0; k < K; ++k) mean += h[k] * signatures[(size_t)k * V + v];
    return mean;
}

// The resamples' plan and the outputs of a bootstrap refit call (include/salnmf.h: salnmf_refit_exposures)
struct BootstrapRun {
    int R, Q;
    int chunk;  // resamples per chunk (bootstrap_chunk)
    uint64_t seed;
    const std::vector<uint32_t>& icounts;  // check_resamples'
    RefitReduceArgs& red;                  // its index filled by check_resamples
    int cus;
    double *exposures, *errors;
    int *n_iterations, *converged;
    double *exposures_quantiles, *exposures_mean;
    int* n_iterations_resampled;
    double *errors_resampled, *exposures_resampled, *timings;
};

// Resamples per chunk: the [chunk][N][V] buffer stays within chunk_bytes (at least one resample); 0 without resamples
inline int bootstrap_chunk(int64_t chunk_bytes, int64_t N, int V, int R) {
    return R > 0 ? (int)chunk_rows(chunk_bytes, sizeof(double) * (size_t)N * V, R) : 0;
}

// The refit of the observed rows and of R resamples of them, chunk by chunk, and the resamples' reduction.  `a` holds what the
// caller uploaded (X [N][V], W, the model's own arrays -- tiled max(chunk, 1) times where they are per problem), P = N and the
// iteration arguments; `inputs_ok` says those uploads succeeded; launch(args, cus, stream) runs the model's tile-solve kernel.
// Span groups: resample, refit, reduce; timings[3] is the number of chunks.
template <typename Args, typename Launch>
int bootstrap_refit(DevBufs& d, const char* what, bool inputs_ok, Args a, const BootstrapRun& io, Launch&& launch) {
    const int64_t N = a.P;
    const int V = a.V, K = a.K, R = io.R, Q = io.Q, chunk = io.chunk;
    const size_t NR = (size_t)N * (size_t)std::max(R, 1);
    a.H = d.get<double>((size_t)N * K);
    a.err = d.get<double>((size_t)N);
    a.nit = d.get<int>((size_t)N);
    a.conv = d.get<int>((size_t)N);
    a.next_tile = d.get<unsigned>(1);
    if (!inputs_ok || !a.H || !a.err || !a.nit || !a.conv || !a.next_tile) return fail("hipMalloc failed (%s of %lld samples)", what, (long long)N);
    uint32_t* dcounts = nullptr;
    double *dXr = nullptr, *dHr = nullptr, *derr_r = nullptr, *dquant = nullptr, *dmean = nullptr;
    int *dnit_r = nullptr, *dconv_r = nullptr;
    if (R > 0) {
        dcounts = upload(d, io.icounts);
        dXr = d.get<double>((size_t)chunk * N * V);
        dHr = d.get<double>(NR * K);
        derr_r = d.get<double>(NR);
        dnit_r = d.get<int>(NR);
        dconv_r = d.get<int>(NR);
        dquant = d.get<double>((size_t)std::max(Q, 1) * N * K);
        dmean = d.get<double>((size_t)N * K);
        if (!dcounts || !dXr || !dHr || !derr_r || !dnit_r || !dconv_r || !dquant || !dmean)
            return fail("hipMalloc failed (%d resamples of %lld x %d, %d signatures)", R, (long long)N, V, K);
    }

    Spans sp;  // resample, refit, reduce
    sp.start(d, io.timings != nullptr);
    CK(sp.timed(1, [&] { return launch(a, io.cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < R; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, R - first);
        CK(sp.timed(0, [&]() -> int {
            refit_launch_resample(dcounts, dXr, N, V, io.seed, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        Args c = a;
        c.X = dXr;
        c.P = (int64_t)count * N;
        c.H = dHr + (size_t)first * N * K;
        c.err = derr_r + (size_t)first * N;
        c.nit = dnit_r + (size_t)first * N;
        c.conv = dconv_r + (size_t)first * N;
        CK(sp.timed(1, [&] { return launch(c, io.cus, d.stream); }));
    }
    if (R > 0) {
        CK(sp.timed(2, [&]() -> int {
            refit_launch_reduce(io.red, dHr, dquant, dmean, N, K, R, Q, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (Q > 0) CK(download(d, io.exposures_quantiles, dquant, (size_t)Q * N * K));
        CK(download(d, io.exposures_mean, dmean, (size_t)N * K));
        CK(download(d, io.n_iterations_resampled, dnit_r, NR));
        CK(download(d, io.errors_resampled, derr_r, NR));
        if (io.exposures_resampled) CK(download(d, io.exposures_resampled, dHr, NR * K));
    }
    CK(download(d, io.exposures, a.H, (size_t)N * K));
    CK(download(d, io.errors, a.err, (size_t)N));
    CK(download(d, io.n_iterations, a.nit, (size_t)N));
    CK(download(d, io.converged, a.conv, (size_t)N));
    HIPCK(hipStreamSynchronize(d.stream));
    CK(sp.totals(3, io.timings));
    if (io.timings) io.timings[3] = (double)n_chunks;
    return 0;
}

// The draws' plan and the outputs of a goodness-of-fit call (include/salnmf.h: salnmf_goodness_of_fit)
struct GofRun {
    int B;
    int chunk;  // draws per chunk: chunk_rows of the [chunk][N][V] buffer
    int cus;
    double *exposures, *errors;
    int *n_iterations, *converged, *n_exceed;
    double *null_mean, *null_errors;
    int* null_n_iterations;
    double *draws, *timings;
};

// The refit of the observed rows, B draws from the fitted model refitted chunk by chunk, and the count of exceedances.  `a`,
// `inputs_ok` and `launch` as bootstrap_refit's (per-problem arrays tiled `chunk` times); draw(H, out, first, count) writes draws
// first .. first + count - 1 from the device-resident exposures H of the observed refit as out[count][N][V], clipped to EPSILON;
// before_wait() is called after the last download and before the stream is waited for (a caller's own download).
// Span groups: draw, refit, reduce; timings[3] is the number of chunks.
template <typename Args, typename Launch, typename Draw, typename BeforeWait>
int gof_run(DevBufs& d, bool inputs_ok, Args a, const GofRun& io, Launch&& launch, Draw&& draw, BeforeWait&& before_wait) {
    const int64_t N = a.P;
    const int V = a.V, K = a.K, B = io.B, chunk = io.chunk;
    const size_t NV = (size_t)N * V, NK = (size_t)N * K, NB = (size_t)N * B;
    a.H = d.get<double>(NK);
    a.err = d.get<double>((size_t)N);
    a.nit = d.get<int>((size_t)N);
    a.conv = d.get<int>((size_t)N);
    a.next_tile = d.get<unsigned>(1);
    double* dXb = d.get<double>((size_t)chunk * NV);
    double* dHb = d.get<double>((size_t)chunk * NK);
    double* derr_b = d.get<double>(NB);
    int* dnit_b = d.get<int>(NB);
    int* dconv_b = d.get<int>((size_t)chunk * N);
    int* dexceed = d.get<int>((size_t)N);
    double* dmean = d.get<double>((size_t)N);
    if (!inputs_ok || !a.H || !a.err || !a.nit || !a.conv || !a.next_tile || !dXb || !dHb || !derr_b || !dnit_b || !dconv_b || !dexceed || !dmean)
        return fail("hipMalloc failed (%d draws of %lld x %d, %d signatures)", B, (long long)N, V, K);

    Spans sp;  // draw, refit, reduce
    sp.start(d, io.timings != nullptr);
    CK(sp.timed(1, [&] { return launch(a, io.cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < B; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, B - first);
        CK(sp.timed(0, [&]() -> int {
            draw(a.H, dXb, first, count);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (io.draws) CK(download(d, io.draws + (size_t)first * NV, dXb, (size_t)count * NV));
        Args c = a;
        c.X = dXb;
        c.P = (int64_t)count * N;
        c.H = dHb;
        c.err = derr_b + (size_t)first * N;
        c.nit = dnit_b + (size_t)first * N;
        c.conv = dconv_b;
        CK(sp.timed(1, [&] { return launch(c, io.cus, d.stream); }));
    }
    const GofReduceArgs red{a.err, derr_b, dexceed, dmean, N, B};
    CK(sp.timed(2, [&]() -> int {
        gof_launch_reduce(red, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    CK(download(d, io.exposures, a.H, NK));
    CK(download(d, io.errors, a.err, (size_t)N));
    CK(download(d, io.n_iterations, a.nit, (size_t)N));
    CK(download(d, io.converged, a.conv, (size_t)N));
    CK(download(d, io.n_exceed, dexceed, (size_t)N));
    CK(download(d, io.null_mean, dmean, (size_t)N));
    CK(download(d, io.null_errors, derr_b, NB));
    CK(download(d, io.null_n_iterations, dnit_b, NB));
    CK(before_wait());
    HIPCK(hipStreamSynchronize(d.stream));
    if (io.draws)  // plain counts: the clipped zeros restored to 0
        for (size_t i = 0; i < (size_t)B * NV; ++i)
            if (io.draws[i] < 1.0) io.draws[i] = 0.0;
    CK(sp.totals(3, io.timings));
    if (io.timings) io.timings[3] = (double)n_chunks;
    return 0;
}

// ---- the assignment (include/salnmf.h: salnmf_assign_signatures_ex, salnmf_nb_assign_signatures; DESIGN.md sections 14.1 and 25)

// What the refit, the assignment, the goodness-of-fit test and the pair calls check and prepare before any launch: the checks of
// salnmf_host_kit.h in their order, with the assignment's sets between the ranges and the signatures, then the device and its CU count.
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

// own_checks() runs between the sets and the signatures: an entry point's checks of its model's own inputs (the dispersions)
template <typename OwnChecks>
int refit_prepare(int device, const double* counts, int64_t N, int V, const double* signatures, int K, int R, int Q, const double* quantiles,
                  int min_iterations, int max_iterations, int conv_test_freq, double tol, bool resample_outputs, RefitInputs& in, const AssignSets& sets,
                  OwnChecks&& own_checks) {
    CK(check_refit_ranges(N, V, K, R, min_iterations, max_iterations, conv_test_freq, tol, Q, resample_outputs));
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
    CK(own_checks());
    CK(check_signatures(signatures, K, V));
    CK(clip_counts(counts, N, V, in.x));
    if (R > 0) CK(check_resamples(counts, N, V, R, Q, quantiles, in.icounts, in.red.index));
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    in.cus = prop.multiProcessorCount;
    return 0;
}

inline int refit_prepare(int device, const double* counts, int64_t N, int V, const double* signatures, int K, int R, int Q, const double* quantiles,
                         int min_iterations, int max_iterations, int conv_test_freq, double tol, bool resample_outputs, RefitInputs& in,
                         const AssignSets& sets = AssignSets{}) {
    return refit_prepare(device, counts, N, V, signatures, K, R, Q, quantiles, min_iterations, max_iterations, conv_test_freq, tol, resample_outputs, in,
                         sets, [] { return 0; });
}

// What an assignment entry point checks before refit_prepare: the outputs, the threshold and the rule that lets the solves of one
// wave's problems follow one another with their tests on the same iterations
struct AssignOutputs {
    double* exposures;
    int* active;
    double* errors;
    int* removal_round;
    double* kl_increase;
    int* n_trials;
    int64_t* n_iterations;
    int* converged;
    double *dense_exposures, *dense_errors;
    int *dense_n_iterations, *dense_converged;
    double *selection_frequency, *exposures_quantiles, *exposures_mean, *exposures_resampled;
    int* readd_round;
    double *kl_decrease, *timings;
};

inline int assign_check(const AssignOutputs& o, bool inputs, int readd, double max_kl_increase, int max_iterations, int conv_test_freq) {
    if (!inputs || !o.exposures || !o.active || !o.errors || !o.removal_round || !o.kl_increase || !o.n_trials || !o.n_iterations || !o.converged ||
        !o.dense_exposures || !o.dense_errors || !o.dense_n_iterations || !o.dense_converged)
        return fail("null argument");
    if (readd == 1 && (!o.readd_round || !o.kl_decrease)) return fail("null output for the re-addition pass");
    if (!std::isfinite(max_kl_increase)) return fail("max_kl_increase must be finite, got %g", max_kl_increase);
    // (solves follow one another inside one wave, and the tests of its 16 problems must fall on the same iterations)
    if (conv_test_freq >= 1 && max_iterations >= 0 && max_iterations % conv_test_freq != 0)
        return fail("max_iterations must be a multiple of conv_test_freq, got %d and %d", max_iterations, conv_test_freq);
    return 0;
}

// The assignment of the observed rows and of R resamples of them, chunk by chunk, the resamples' reduction and their selection
// frequencies.  `a` holds what the caller uploaded (X [N][V], W, the model's own arrays), P = N, V, K, the iteration arguments,
// the threshold and readd; `inputs_ok` says those uploads succeeded; launch(args, cus, stream) runs the model's assignment kernel.
// Span groups: resample, assign, reduce; timings[3] is the number of chunks.
template <typename Args, typename Launch>
int assign_run(DevBufs& d, bool inputs_ok, Args a, RefitInputs& in, int R, int Q, uint64_t seed, int64_t chunk_bytes, const AssignOutputs& o,
               Launch&& launch) {
    const int64_t N = a.P;
    const int V = a.V, K = a.K, cus = in.cus, readd = a.readd;
    const int chunk = bootstrap_chunk(chunk_bytes, N, V, R);
    const size_t NK = (size_t)N * K, NR = (size_t)N * (size_t)std::max(R, 1);
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
    if (!inputs_ok || !dH || !dHd || !dkl || !dact || !dround || !derr || !derr_d || !dnit || !dconv || !dntr || !dnit_d || !dconv_d || !dnext)
        return fail("hipMalloc failed (assignment of %lld samples)", (long long)N);
    uint32_t *dcand = nullptr, *dreq = nullptr;
    int* drround = nullptr;
    double* dkld = nullptr;
    const bool candidates = !in.cand.empty(), required = !in.req.empty();
    if (candidates) dcand = upload(d, in.cand);
    if (required) dreq = upload(d, in.req);
    if (readd) drround = d.get<int>(NK), dkld = d.get<double>(NK);
    if ((candidates && !dcand) || (required && !dreq) || (readd && (!drround || !dkld))) return fail("hipMalloc failed (sets of %lld samples)", (long long)N);
    uint32_t* dcounts = nullptr;
    double *dXr = nullptr, *dHr = nullptr, *derr_r = nullptr, *dquant = nullptr, *dmean = nullptr, *dfreq = nullptr;
    long long* dnit_r = nullptr;
    int *dconv_r = nullptr, *dntr_r = nullptr;
    if (R > 0) {
        dcounts = upload(d, in.icounts);
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
    }

    a.H = dH, a.err = derr, a.nit = dnit, a.conv = dconv, a.ntrials = dntr, a.active = dact, a.round = dround, a.kl = dkl;
    a.dH = dHd, a.derr = derr_d, a.dnit = dnit_d, a.dconv = dconv_d, a.next_tile = dnext;
    a.cand = dcand, a.req = dreq, a.rround = drround, a.kld = dkld, a.N = N;
    Spans sp;  // resample, assign, reduce
    sp.start(d, o.timings != nullptr);
    CK(sp.timed(1, [&] { return launch(a, cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < R; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, R - first);
        CK(sp.timed(0, [&]() -> int {
            refit_launch_resample(dcounts, dXr, N, V, seed, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        // a resample's problems keep their exposures only: no per-signature record, no phase-0 copy
        Args c = a;
        c.X = dXr;
        c.P = (int64_t)count * N;
        c.H = dHr + (size_t)first * NK;
        c.err = derr_r + (size_t)first * N;
        c.nit = dnit_r + (size_t)first * N;
        c.conv = dconv_r + (size_t)first * N;
        c.ntrials = dntr_r + (size_t)first * N;
        c.active = nullptr, c.round = nullptr, c.kl = nullptr, c.rround = nullptr, c.kld = nullptr;
        c.dH = nullptr, c.derr = nullptr, c.dnit = nullptr, c.dconv = nullptr;
        CK(sp.timed(1, [&] { return launch(c, cus, d.stream); }));
    }
    if (R > 0) {
        CK(sp.timed(2, [&]() -> int {
            refit_launch_reduce(in.red, dHr, dquant, dmean, N, K, R, Q, d.stream);
            HIPCK(hipGetLastError());
            assign_launch_selection(dHr, dfreq, (int64_t)NK, R, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (Q > 0) CK(download(d, o.exposures_quantiles, dquant, (size_t)Q * NK));
        CK(download(d, o.exposures_mean, dmean, NK));
        CK(download(d, o.selection_frequency, dfreq, NK));
        if (o.exposures_resampled) CK(download(d, o.exposures_resampled, dHr, NR * K));
    }
    CK(download(d, o.exposures, dH, NK));
    CK(download(d, o.active, dact, NK));
    CK(download(d, o.removal_round, dround, NK));
    CK(download(d, o.kl_increase, dkl, NK));
    if (readd) {
        CK(download(d, o.readd_round, drround, NK));
        CK(download(d, o.kl_decrease, dkld, NK));
    }
    CK(download(d, o.errors, derr, (size_t)N));
    CK(download(d, o.n_trials, dntr, (size_t)N));
    CK(download(d, o.n_iterations, dnit, (size_t)N));
    CK(download(d, o.converged, dconv, (size_t)N));
    CK(download(d, o.dense_exposures, dHd, NK));
    CK(download(d, o.dense_errors, derr_d, (size_t)N));
    CK(download(d, o.dense_n_iterations, dnit_d, (size_t)N));
    CK(download(d, o.dense_converged, dconv_d, (size_t)N));
    HIPCK(hipStreamSynchronize(d.stream));
    CK(sp.totals(3, o.timings));
    if (o.timings) o.timings[3] = (double)n_chunks;
    return 0;
}

// B draws from a fitted model into out [B][N][V] on the host, through a chunk buffer of the default budget: draw(out, first,
// count) writes draws first .. first + count - 1 as out[count][N][V].  `inputs_ok` says the caller's uploads succeeded.  The
// copies are not waited for: the caller does that, after any download of its own.
template <typename Draw>
int draw_run(DevBufs& d, bool inputs_ok, int64_t N, int V, int B, double* out, Draw&& draw) {
    const size_t NV = (size_t)N * V;
    const int chunk = (int)chunk_rows(0, sizeof(double) * NV, B);
    double* dout = d.get<double>((size_t)chunk * NV);
    if (!inputs_ok || !dout) return fail("hipMalloc failed (%d draws of %lld x %d)", chunk, (long long)N, V);
    for (int first = 0; first < B; first += chunk) {
        const int count = std::min(chunk, B - first);
        draw(dout, first, count);
        HIPCK(hipGetLastError());
        CK(download(d, out + (size_t)first * NV, dout, (size_t)count * NV));
    }
    return 0;
}

// ---- the pair run: what the presence test (salnmf_presence.h), its negative-binomial counterpart
// (salnmf_nb_presence.h, section 26), its power analysis (salnmf_power.h, section 18) and the profile likelihood with its intervals
// (salnmf_profile.h, section 19) do alike.  All run pair_observed; the presence tests go on with their draws (presence_enqueue,
// pair_draw_solve) and presence_finish, the power analysis putting its launches on the same stream in between.
//
// The two models differ in the kernel's argument struct (PresenceArgs, or NbPresenceArgs which extends it), and in a MODEL object:
//   int  own_checks()                          the model's own inputs, at refit_prepare's place for them (the dispersions)
//   bool inputs(DevBufs&, Args&)               uploads the model's own arrays and sets their fields of the arguments
//   int  launch(const Args&, cus, stream)      the model's two-solve kernel
//   int  after_observed(io, run)               between the observed launch and the first draw (the bound on the null fit's mean)
//   void draw(run, seed, first, count)         draws first .. first + count - 1 of every pair into run.dXb, [count][pairs][V]
//   int  before_wait(DevBufs&)                 after the last download of the driver (a download of the model's own)

// The arguments of a pair call.  The first group is every call's; the second the presence test's (null and 0 in a profile call).
struct PairIO {
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

    int B;
    uint64_t seed;
    int64_t chunk_bytes;
    double* statistic;
    int* n_exceed;
    double *null_mean, *null_exposures, *null_errors;
    int *n_iterations, *converged;
    double* null_statistics;
    int* null_n_iterations;
    double* draws;
};

// What a call keeps between its launches and its results: the pair list, the observed fits of every pair on the host (stat =
// f0 - f1, f = (f1, f0), H1), the device buffers later launches read again and the host ends of the asynchronous copies (which
// live until d's destructor has waited for the stream: d is the last member, and exists once the validation has passed and a
// pair is tested).
template <typename Args>
struct PairRunOf {
    RefitInputs in;
    std::vector<int> pair_n, pair_s;
    std::vector<size_t> slot;  // pair j is entry slot[j] of the (N, S) results
    std::vector<double> h_stat, h_f, h_H1;
    std::vector<double> h_H0, h_mean, h_stat_b, h_draws;  // the presence test's
    std::vector<int> h_nit, h_conv, h_exceed, h_nit_b;
    Spans sp;  // presence: draw, solve, reduce; planting, alternative draw, solve, reduce.  profile: the observed launch, the profile launch
    size_t NP = 0;
    int64_t chunk_rows = 0;  // rows [pairs][V] of the chunk buffer that chunk_bytes allows
    int n_chunks = 0;
    bool h0_on_host = false;  // the model's after_observed has copied dH0 into h_H0 and waited for it
    double *dW = nullptr, *dX = nullptr, *dH0 = nullptr, *dstat_b = nullptr, *dXb = nullptr;
    int *dpn = nullptr, *dps = nullptr;
    uint32_t* dcand = nullptr;
    Args a{};  // the observed launch's
    std::unique_ptr<DevBufs> d;
};

inline int presence_check_test(const int* test, int S, int K) {
    if (S < 1 || S > REFIT_KMAX) return fail("n_test must be in [1, %d], got %d", REFIT_KMAX, S);
    for (int j = 0; j < S; ++j) {
        if (test[j] < 0 || test[j] >= K) return fail("tested signature %d is not in [0, %d)", test[j], K);
        for (int i = 0; i < j; ++i)
            if (test[i] == test[j]) return fail("signature %d is tested twice", test[j]);
    }
    return 0;
}

// The tested pairs, sample after sample: s is a candidate and not the only one.  Pair j is entry slot[j] of the (N, S) results.
inline void presence_list_pairs(const RefitInputs& in, int64_t N, int K, const int* test, int S, bool with_candidates, uint8_t* tested,
                                std::vector<int>& pair_n, std::vector<int>& pair_s, std::vector<size_t>& slot) {
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

// What follows a call's own null checks: the rest of the validation (integer counts only where draws will be made of them), the
// pair list, the untested entries of the alternative fit, and -- with a tested pair -- the uploads and the observed launch under
// span `span`: the alternative solve on C, then the null solve (which is the frozen solve at 0.0), and the copies of stat, f and
// H1 back.  Nothing is waited for; h0 (r.dH0, [pairs][K]) stays on the device.
template <typename Args, typename Model>
int pair_observed(const PairIO& io, bool integer_counts, int span, PairRunOf<Args>& r, Model& m) {
    const int64_t N = io.N;
    const int V = io.V, K = io.K, S = io.S;
    if (io.conv_test_freq >= 1 && io.max_iterations >= 0 && io.max_iterations % io.conv_test_freq != 0)
        return fail("max_iterations must be a multiple of conv_test_freq, got %d and %d", io.max_iterations, io.conv_test_freq);
    CK(presence_check_test(io.test, S, K));
    RefitInputs& in = r.in;
    CK(refit_prepare(io.device, io.counts, N, V, io.signatures, K, 0, 0, nullptr, io.min_iterations, io.max_iterations, io.conv_test_freq, io.tol, true,
                     in, AssignSets{io.candidates, nullptr, 0}, [&] { return m.own_checks(); }));
    if (integer_counts) CK(refit_check_counts(io.counts, N, V, in.icounts));  // row totals below 2^32 too (the values themselves are not used)
    presence_list_pairs(in, N, K, io.test, S, io.candidates != nullptr, io.tested, r.pair_n, r.pair_s, r.slot);
    const size_t NP = r.NP = r.pair_n.size();
    if (NP > 0x7fffffff) return fail("%zu tested pairs: at most 2^31 - 1", NP);
    const double nan = std::nan("");
    std::fill(io.exposures, io.exposures + (size_t)N * K, nan);
    std::fill(io.errors, io.errors + N, nan);
    if (NP == 0) return 0;

    const size_t PK = NP * K;
    r.h_stat.resize(NP), r.h_f.resize(2 * NP), r.h_H1.resize(PK);
    r.d.reset(new DevBufs);
    DevBufs& d = *r.d;
    CK(d.own_stream());
    r.dW = upload(d, io.signatures, (size_t)K * V);
    r.dX = upload(d, in.x);
    r.dpn = upload(d, r.pair_n);
    r.dps = upload(d, r.pair_s);
    r.dcand = io.candidates ? upload(d, in.cand) : nullptr;
    double* dstat = d.get<double>(NP);
    double* df = d.get<double>(2 * NP);
    int* dnit = d.get<int>(2 * NP);
    int* dconv = d.get<int>(2 * NP);
    double* dH1 = d.get<double>(PK);
    r.dH0 = d.get<double>(PK);
    unsigned* dnext = d.get<unsigned>(1);
    r.a = Args{};
    static_cast<PresenceArgs&>(r.a) = PresenceArgs{r.dX, r.dW, r.dpn, r.dps, r.dcand, dstat, dnit, df, dconv, dH1, r.dH0, dnext, (int64_t)NP, (int64_t)NP, V, K, 1,
                                                   io.min_iterations, io.max_iterations, io.conv_test_freq, io.tol};
    const bool model_ok = m.inputs(d, r.a);
    if (!r.dW || !r.dX || !r.dpn || !r.dps || !dstat || !df || !dnit || !dconv || !dH1 || !r.dH0 || !dnext || (io.candidates && !r.dcand) || !model_ok)
        return fail("hipMalloc or upload failed (%zu pairs x %d, %d signatures)", NP, V, K);
    r.sp.start(d, io.timings != nullptr);
    CK(r.sp.timed(span, [&] { return m.launch(r.a, in.cus, d.stream); }));
    CK(download(d, r.h_stat, dstat));
    CK(download(d, r.h_f, df));
    CK(download(d, r.h_H1, dH1));
    return 0;
}

// (after the stream has been waited for) a sample's alternative fit is that of its first tested pair: every tested pair of a
// sample solves the same problem on C and holds the same bits
template <typename Args>
void pair_scatter_alternative(const PairIO& io, const PairRunOf<Args>& r) {
    const int K = io.K;
    for (size_t j = 0; j < r.NP; ++j)
        if (j == 0 || r.pair_n[j - 1] != r.pair_n[j]) {
            const size_t n = (size_t)r.pair_n[j];
            std::copy(r.h_H1.begin() + j * K, r.h_H1.begin() + (j + 1) * K, io.exposures + n * K);
            io.errors[n] = r.h_f[2 * j];
        }
}

// Draw rows first .. of `rows` into the chunk buffer (draw(first, count) launches the draw of `count` rows [pairs][V] into
// r.dXb), `chunk` at a time, and solve them as the observed launch solved the counts: a draw's problems keep their statistic
// (stat [rows][pairs]) and iteration counts (nit [rows][pairs][2]) only.  host_copy, if not null, gets the drawn rows.
template <typename Args, typename Model, typename Draw>
int pair_draw_solve(PairRunOf<Args>& r, Model& m, int64_t rows, int64_t chunk, Draw&& draw, double* stat, int* nit, double* host_copy, int span_draw,
                    int span_solve, int* n_chunks) {
    DevBufs& d = *r.d;
    const size_t NP = r.NP, PV = NP * r.a.V;
    for (int64_t first = 0; first < rows; first += chunk, ++*n_chunks) {
        const int64_t count = std::min(chunk, rows - first);
        CK(r.sp.timed(span_draw, [&]() -> int {
            draw(first, count);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (host_copy) CK(download(d, host_copy + (size_t)first * PV, r.dXb, (size_t)count * PV));
        Args c = r.a;
        c.X = r.dXb;
        c.by_sample = 0;
        c.P = count * (int64_t)NP;
        c.stat = stat + (size_t)first * NP;
        c.nit = nit + 2 * (size_t)first * NP;
        c.f = nullptr, c.conv = nullptr, c.H1 = nullptr, c.H0 = nullptr;
        CK(r.sp.timed(span_solve, [&] { return m.launch(c, r.in.cus, d.stream); }));
    }
    return 0;
}

// Validation, the pair list, the untested entries of the results, and -- with a tested pair -- everything the presence test puts
// on the stream: pair_observed, the null chunks, the reduction and the downloads.  Nothing is waited for (unless the model's
// after_observed does).  The null statistics (r.dstat_b, [B][pairs]) stay on the device; the chunk buffer r.dXb holds
// min(max(B, other_rows), r.chunk_rows) rows, so that a caller with other_rows draws of its own can reuse it.
template <typename Args, typename Model>
int presence_enqueue(const PairIO& io, int64_t other_rows, PairRunOf<Args>& r, Model& m) {
    const int64_t N = io.N;
    const int V = io.V, K = io.K, S = io.S, B = io.B;
    if (!io.counts || !io.signatures || !io.test || !io.tested || !io.statistic || !io.n_exceed || !io.null_mean || !io.exposures || !io.errors ||
        !io.null_exposures || !io.null_errors || !io.n_iterations || !io.converged || !io.null_statistics || !io.null_n_iterations)
        return fail("null argument");
    CK(check_n_draws(B));
    CK(pair_observed(io, true, 1, r, m));
    const size_t NS = (size_t)N * S, NP = r.NP;
    const double nan = std::nan("");
    std::fill(io.statistic, io.statistic + NS, nan);
    std::fill(io.null_mean, io.null_mean + NS, nan);
    std::fill(io.null_errors, io.null_errors + NS, nan);
    std::fill(io.n_exceed, io.n_exceed + NS, 0);
    std::fill(io.null_exposures, io.null_exposures + NS * K, nan);
    std::fill(io.n_iterations, io.n_iterations + 2 * NS, 0);
    std::fill(io.converged, io.converged + 2 * NS, 0);
    std::fill(io.null_statistics, io.null_statistics + (size_t)B * NS, nan);
    std::fill(io.null_n_iterations, io.null_n_iterations + 2 * (size_t)B * NS, 0);
    if (io.draws) std::fill(io.draws, io.draws + (size_t)B * NS * V, 0.0);
    if (io.timings) io.timings[0] = io.timings[1] = io.timings[2] = io.timings[3] = 0.0;
    if (NP == 0) return 0;

    // draws per chunk: the [chunk][pairs][V] buffer stays within chunk_bytes (at least one draw)
    const size_t PV = NP * V, PK = NP * K, PB = NP * B;
    r.chunk_rows = chunk_rows(io.chunk_bytes, sizeof(double) * PV, INT64_MAX);
    const int64_t buffer_rows = std::min<int64_t>(std::max<int64_t>(B, other_rows), r.chunk_rows);
    r.h_H0.resize(PK), r.h_mean.resize(NP), r.h_stat_b.resize(PB), r.h_draws.resize(io.draws ? PB * V : 0);
    r.h_nit.resize(2 * NP), r.h_conv.resize(2 * NP), r.h_exceed.resize(NP), r.h_nit_b.resize(2 * PB);
    CK(m.after_observed(io, r));
    DevBufs& d = *r.d;
    r.dXb = d.get<double>((size_t)buffer_rows * PV);
    r.dstat_b = d.get<double>(PB);
    int* dnit_b = d.get<int>(2 * PB);
    int* dexceed = d.get<int>(NP);
    double* dmean = d.get<double>(NP);
    if (!r.dXb || !r.dstat_b || !dnit_b || !dexceed || !dmean) return fail("hipMalloc failed (%d draws of %zu pairs x %d, %d signatures)", B, NP, V, K);
    // from the device-resident exposures of the observed null fits
    CK(pair_draw_solve(r, m, B, std::min<int64_t>(B, r.chunk_rows), [&](int64_t first, int64_t count) { m.draw(r, io.seed, (int)first, (int)count); },
                       r.dstat_b, dnit_b, io.draws ? r.h_draws.data() : nullptr, 0, 1, &r.n_chunks));
    // gof_reduce_kernel over the pairs: n_exceed counts t_b >= t (false for a NaN on either side), null_mean sums from 0.0 in ascending b
    const GofReduceArgs red{r.a.stat, r.dstat_b, dexceed, dmean, (int64_t)NP, B};
    CK(r.sp.timed(2, [&]() -> int {
        gof_launch_reduce(red, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    CK(download(d, r.h_nit, r.a.nit));
    CK(download(d, r.h_conv, r.a.conv));
    if (!r.h0_on_host) CK(download(d, r.h_H0, r.dH0));
    CK(download(d, r.h_exceed, dexceed));
    CK(download(d, r.h_mean, dmean));
    CK(download(d, r.h_stat_b, r.dstat_b));
    CK(download(d, r.h_nit_b, dnit_b));
    CK(m.before_wait(d));
    return 0;
}

// Waits for the stream, then the compact pair list back into the (N, S) results and the first four timings.
template <typename Args>
int presence_finish(const PairIO& io, PairRunOf<Args>& r) {
    const int V = io.V, K = io.K, B = io.B;
    const size_t NP = r.NP, NS = (size_t)io.N * io.S;
    HIPCK(hipStreamSynchronize(r.d->stream));
    pair_scatter_alternative(io, r);
    for (size_t j = 0; j < NP; ++j) {
        const size_t o = r.slot[j];
        io.statistic[o] = r.h_stat[j];
        io.n_exceed[o] = r.h_exceed[j];
        io.null_mean[o] = r.h_mean[j];
        io.null_errors[o] = r.h_f[2 * j + 1];
        std::copy(r.h_H0.begin() + j * K, r.h_H0.begin() + (j + 1) * K, io.null_exposures + o * K);
        for (int i = 0; i < 2; ++i) io.n_iterations[2 * o + i] = r.h_nit[2 * j + i], io.converged[2 * o + i] = r.h_conv[2 * j + i];
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
    CK(r.sp.totals(3, io.timings));
    if (io.timings) io.timings[3] = (double)r.n_chunks;
    return 0;
}

}  // namespace salnmf
