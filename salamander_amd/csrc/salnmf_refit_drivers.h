// The three host drivers that the Poisson entry points (salnmf_refit.hip: salnmf_refit_exposures, salnmf_goodness_of_fit,
// salnmf_draw_model_counts) and their negative-binomial counterparts (salnmf_nb.hip) share, DESIGN.md section 13.1.  The two
// sides differ in the kernel's argument struct (RefitArgs, NbRefitArgs), its launcher and the draw call, so each driver is a
// template over those and an entry point is its checks, the uploads of its model's own inputs and one call.  Host code only:
// no kernel is defined or named here.  A driver issues its launches, memsets and copies in one fixed order on d's stream;
// tests/test_gpu_refit_family_bits.py and tests/test_gpu_nb_family_bits.py hold both sides to the bits that order gives.
#pragma once
#include "salnmf_host_kit.h"

namespace salnmf {

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
