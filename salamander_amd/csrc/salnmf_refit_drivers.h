// The four host drivers that the Poisson entry points (salnmf_refit.hip: salnmf_refit_exposures, salnmf_goodness_of_fit,
// salnmf_draw_model_counts, salnmf_assign_signatures_ex) and their negative-binomial counterparts (salnmf_nb.hip, and
// salnmf_nb_assign.hip for the assignment) share, DESIGN.md section 13.1.  The two sides differ in the kernel's argument struct
// (RefitArgs, NbRefitArgs; AssignArgs, NbAssignArgs), its launcher and the draw call, so each driver is a
// template over those and an entry point is its checks, the uploads of its model's own inputs and one call.  Host code only:
// no kernel is defined or named here.  A driver issues its launches, memsets and copies in one fixed order on d's stream;
// tests/test_gpu_refit_family_bits.py and tests/test_gpu_nb_family_bits.py hold both sides to the bits that order gives.
#pragma once
#include "salnmf_host_kit.h"
#include "salnmf_assign.h"
#include "salnmf_nb.h"

namespace salnmf {

// The dispersions of a negative-binomial entry point: one per sample, finite and in (0, NB_ALPHA_MAX]
inline int nb_check_dispersion(const double* dispersion, int64_t N) {
    for (int64_t n = 0; n < N; ++n)
        if (!std::isfinite(dispersion[n]) || !(dispersion[n] > 0.0) || dispersion[n] > NB_ALPHA_MAX)
            return fail("dispersion must be finite and in (0, %g]: sample %lld holds %g", NB_ALPHA_MAX, (long long)n, dispersion[n]);
    return 0;
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

}  // namespace salnmf
