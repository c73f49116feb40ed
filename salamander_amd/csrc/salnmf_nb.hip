// Host side of the negative-binomial refit (include/salnmf.h: salnmf_nb_refit_exposures) and the instantiations of its kernel
// (salnmf_nb.h: nb_refit_kernel), DESIGN.md section 23.  A translation unit of its own, as section 20's: the tile-solve kernels of
// salnmf_refit.hip fill the register file, and nothing added here can move their allocation -- that object is compiled from
// unchanged input.  The driver is written with the refit family's host kit (salnmf_host_kit.h: Spans, chunk_rows, upload /
// download) and reuses the resamples' machinery: refit_check_counts and refit_launch_resample (salnmf_batch.hip) draw them, and
// refit_reduce_kernel reduces them.  Also the drivers of the draw from the fitted negative-binomial model and of the goodness-of-fit
// test on it (salnmf_draw_nb_counts, salnmf_nb_goodness_of_fit): nb_draw_kernel and gof_reduce_kernel are
// salnmf_batch.hip's, behind nb_launch_draw (salnmf_nbdraw.h) and gof_launch_reduce (salnmf_gof.h).
#define SALNMF_TEMPLATES_ONLY 1
#define SALNMF_REFIT_KERNELS 1
#define SALNMF_NB_KERNELS 1
#include "../../include/salnmf.h"
#include "salnmf_kernels.h"
#include "salnmf_device.h"
#include "salnmf_host_kit.h"
// salnmf_refit.h's pieces are templates or forced inline, but refit_reduce_kernel is an ordinary kernel that salnmf_refit.hip
// already defines: this unit compiles the same text under a name of its own, so that the two objects link.
#define refit_reduce_kernel nb_refit_reduce_kernel
#include "salnmf_refit.h"
#undef refit_reduce_kernel
#include "salnmf_nb.h"
#include "salnmf_nbdraw.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

using namespace salnmf;

namespace {

// One workgroup per CU (the kernel's registers leave room for one wave per SIMD; waves fetch tiles until the list is empty), the
// list's head reset, and the instantiation for (K + 15) / 16 signature tiles: what salnmf_refit.hip's launch_tiles does
int launch_nb_refit(const NbRefitArgs& a, int cus, hipStream_t stream) {
    const int64_t ntiles = (a.P + 15) / 16;
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)cus, (ntiles + WAVES - 1) / WAVES));
    HIPCK(hipMemsetAsync(a.next_tile, 0, sizeof(unsigned), stream));
    switch ((a.K + 15) / 16) {
        case 1: hipLaunchKernelGGL(nb_refit_kernel<1>, grid, dim3(BLOCK), 0, stream, a); break;
        case 2: hipLaunchKernelGGL(nb_refit_kernel<2>, grid, dim3(BLOCK), 0, stream, a); break;
        case 3: hipLaunchKernelGGL(nb_refit_kernel<3>, grid, dim3(BLOCK), 0, stream, a); break;
        case 4: hipLaunchKernelGGL(nb_refit_kernel<4>, grid, dim3(BLOCK), 0, stream, a); break;
        case 5: hipLaunchKernelGGL(nb_refit_kernel<5>, grid, dim3(BLOCK), 0, stream, a); break;
        case 6: hipLaunchKernelGGL(nb_refit_kernel<6>, grid, dim3(BLOCK), 0, stream, a); break;
        default: return fail("no negative-binomial refit kernel for %d signatures", a.K);
    }
    HIPCK(hipGetLastError());
    return 0;
}

// What every entry point of this unit checks of its problems before any launch, and the clipped counts x = max(counts, EPSILON)
int nb_check(const double* counts, int64_t N, int V, const double* signatures, int K, const double* dispersion, int min_iterations, int max_iterations,
             int conv_test_freq, double tol, std::vector<double>& x) {
    if (N < 1 || N > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)N);
    if (V < 1 || V > VMAX) return fail("n_features must be in [1, %d], got %d", VMAX, V);
    if (K < 1 || K > REFIT_KMAX) return fail("n_signatures must be in [1, %d], got %d", REFIT_KMAX, K);
    if (min_iterations < 0 || max_iterations < min_iterations) return fail("need 0 <= min_iterations <= max_iterations, got %d and %d", min_iterations, max_iterations);
    if (conv_test_freq < 1) return fail("conv_test_freq must be positive, got %d", conv_test_freq);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail("tol must be finite and not negative, got %g", tol);
    for (int64_t n = 0; n < N; ++n)
        if (!std::isfinite(dispersion[n]) || !(dispersion[n] > 0.0) || dispersion[n] > NB_ALPHA_MAX)
            return fail("dispersion must be finite and in (0, %g]: sample %lld holds %g", NB_ALPHA_MAX, (long long)n, dispersion[n]);
    for (int k = 0; k < K; ++k) {
        double sum = 0.0;
        for (int v = 0; v < V; ++v) {
            const double w = signatures[(size_t)k * V + v];
            if (!std::isfinite(w) || w < 0.0) return fail("signature %d, feature %d: entries must be finite and not negative, got %g", k, v, w);
            sum += w;
        }
        if (!(sum > 0.0) || !std::isfinite(sum)) return fail("signature %d needs a positive finite sum", k);
    }
    x.resize((size_t)N * V);
    for (size_t i = 0; i < x.size(); ++i) {
        if (!std::isfinite(counts[i]) || counts[i] < 0.0)
            return fail("counts must be finite and not negative: row %lld, column %d holds %g", (long long)(i / V), (int)(i % V), counts[i]);
        x[i] = counts[i] < SALNMF_EPSILON ? SALNMF_EPSILON : counts[i];
    }
    return 0;
}

// The per-sample constants of the gamma draw (salnmf_nbdraw.h): d = a' - 1/3 and c = 1 / sqrt(9 d), a' = alpha (alpha >= 1) or alpha + 1:
// computed here, so that the kernel's gamma path has no square root of its own
void nb_gamma_constants(const double* dispersion, int64_t N, std::vector<double>& gd, std::vector<double>& gc) {
    gd.resize((size_t)N), gc.resize((size_t)N);
    for (int64_t n = 0; n < N; ++n) {
        const double shape = dispersion[n] >= 1.0 ? dispersion[n] : dispersion[n] + 1.0;
        gd[(size_t)n] = shape - 1.0 / 3.0;
        gc[(size_t)n] = 1.0 / std::sqrt(9.0 * gd[(size_t)n]);
    }
}

int nb_check_draws(int n_draws) {
    if (n_draws < 1 || n_draws > GOF_MAX_DRAWS) return fail("n_draws must be in [1, %d], got %d", GOF_MAX_DRAWS, n_draws);
    return 0;
}

}  // namespace

extern "C" int salnmf_nb_refit_exposures(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                         const double* dispersion, int n_resamples, uint64_t seed, int n_quantiles, const double* quantiles,
                                         int min_iterations, int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes, double* exposures,
                                         double* errors, int* n_iterations, int* converged, double* exposures_quantiles, double* exposures_mean,
                                         int* n_iterations_resampled, double* errors_resampled, double* exposures_resampled, double* timings) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, R = n_resamples, Q = n_quantiles;
    if (!counts || !signatures || !dispersion || !exposures || !errors || !n_iterations || !converged) return fail("null argument");
    if (R < 0 || R > REFIT_SORT_MAX) return fail("n_resamples must be in [0, %d], got %d", REFIT_SORT_MAX, R);
    if (Q < 0 || Q > REFIT_MAX_QUANTILES) return fail("n_quantiles must be in [0, %d], got %d", REFIT_MAX_QUANTILES, Q);
    if (R > 0 && !(exposures_mean && n_iterations_resampled && errors_resampled && (Q <= 0 || (quantiles && exposures_quantiles))))
        return fail("null output for the resamples");
    std::vector<double> x;
    CK(nb_check(counts, N, V, signatures, K, dispersion, min_iterations, max_iterations, conv_test_freq, tol, x));
    std::vector<uint32_t> icounts;
    RefitReduceArgs red{};
    if (R > 0) {
        CK(refit_check_counts(counts, N, V, icounts));
        for (int i = 0; i < Q; ++i) {
            const double qv = quantiles[i];
            if (!(qv >= 0.0 && qv <= 1.0)) return fail("quantile %d must be in [0, 1], got %g", i, qv);
            // an order statistic, taken outward
            const double pos = qv * (double)(R - 1);
            red.index[i] = std::min(R - 1, std::max(0, (int)(qv <= 0.5 ? std::floor(pos) : std::ceil(pos))));
        }
    }
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    const int cus = prop.multiProcessorCount;

    // resamples per chunk: the [chunk][N][V] buffer stays within chunk_bytes (at least one resample); a resample of sample n
    // carries sample n's dispersion, so a chunk's problems read the samples' dispersions repeated `chunk` times
    const int chunk = R > 0 ? (int)chunk_rows(chunk_bytes, sizeof(double) * (size_t)N * V, R) : 0;
    std::vector<double> alpha((size_t)N * (size_t)std::max(chunk, 1));
    for (size_t i = 0; i < alpha.size(); ++i) alpha[i] = dispersion[i % (size_t)N];

    // (host buffers of the asynchronous copies live until d's destructor has waited for the stream)
    DevBufs d;
    CK(d.own_stream());
    const size_t NR = (size_t)N * (size_t)std::max(R, 1);
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dX = upload(d, x);
    double* dalpha = upload(d, alpha);
    double* dH = d.get<double>((size_t)N * K);
    double* derr = d.get<double>((size_t)N);
    int* dnit = d.get<int>((size_t)N);
    int* dconv = d.get<int>((size_t)N);
    unsigned* dnext = d.get<unsigned>(1);
    if (!dW || !dX || !dalpha || !dH || !derr || !dnit || !dconv || !dnext) return fail("hipMalloc failed (negative-binomial refit of %lld samples)", (long long)N);
    uint32_t* dcounts = nullptr;
    double *dXr = nullptr, *dHr = nullptr, *derr_r = nullptr, *dquant = nullptr, *dmean = nullptr;
    int *dnit_r = nullptr, *dconv_r = nullptr;
    if (R > 0) {
        dcounts = upload(d, icounts);
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

    NbRefitArgs a{dX, dW, dalpha, dH, derr, dnit, dconv, dnext, N, V, K, min_iterations, max_iterations, conv_test_freq, tol};
    Spans sp;  // resample, refit, reduce
    sp.start(d, timings != nullptr);
    CK(sp.timed(1, [&] { return launch_nb_refit(a, cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < R; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, R - first);
        CK(sp.timed(0, [&]() -> int {
            refit_launch_resample(dcounts, dXr, N, V, seed, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        NbRefitArgs c = a;
        c.X = dXr;
        c.P = (int64_t)count * N;
        c.H = dHr + (size_t)first * N * K;
        c.err = derr_r + (size_t)first * N;
        c.nit = dnit_r + (size_t)first * N;
        c.conv = dconv_r + (size_t)first * N;
        CK(sp.timed(1, [&] { return launch_nb_refit(c, cus, d.stream); }));
    }
    if (R > 0) {
        red.H = dHr, red.quant = dquant, red.mean = dmean;
        red.N = N, red.K = K, red.R = R, red.Q = Q;
        red.R2 = 1;
        while (red.R2 < R) red.R2 <<= 1;
        CK(sp.timed(2, [&]() -> int {
            hipLaunchKernelGGL(nb_refit_reduce_kernel, dim3((unsigned)N), dim3(REFIT_SORT_BLOCK), 0, d.stream, red);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (Q > 0) CK(download(d, exposures_quantiles, dquant, (size_t)Q * N * K));
        CK(download(d, exposures_mean, dmean, (size_t)N * K));
        CK(download(d, n_iterations_resampled, dnit_r, NR));
        CK(download(d, errors_resampled, derr_r, NR));
        if (exposures_resampled) CK(download(d, exposures_resampled, dHr, NR * K));
    }
    CK(download(d, exposures, dH, (size_t)N * K));
    CK(download(d, errors, derr, (size_t)N));
    CK(download(d, n_iterations, dnit, (size_t)N));
    CK(download(d, converged, dconv, (size_t)N));
    HIPCK(hipStreamSynchronize(d.stream));
    CK(sp.totals(3, timings));
    if (timings) timings[3] = (double)n_chunks;
    return 0;
}

// ---- draws from the fitted negative-binomial model and the goodness-of-fit test on them (salnmf_nbdraw.h)

extern "C" int salnmf_draw_nb_counts(int device, const double* exposures, int64_t n_samples, int n_signatures, const double* signatures, int n_features,
                                     const double* dispersion, int n_draws, uint64_t seed, double* out, int* n_failed) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, B = n_draws;
    if (!exposures || !signatures || !dispersion || !out || !n_failed) return fail("null argument");
    if (N < 1 || N > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)N);
    if (V < 1 || V > GOF_VMAX) return fail("n_features must be in [1, %d], got %d", GOF_VMAX, V);
    if (K < 1 || K > GOF_KMAX) return fail("n_signatures must be in [1, %d], got %d", GOF_KMAX, K);
    CK(nb_check_draws(B));
    for (size_t i = 0; i < (size_t)N * K; ++i)
        if (!std::isfinite(exposures[i]) || exposures[i] < 0.0)
            return fail("exposures must be finite and not negative: row %lld, signature %d holds %g", (long long)(i / K), (int)(i % K), exposures[i]);
    for (size_t i = 0; i < (size_t)K * V; ++i)
        if (!std::isfinite(signatures[i]) || signatures[i] < 0.0)
            return fail("signature %d, feature %d: entries must be finite and not negative, got %g", (int)(i / V), (int)(i % V), signatures[i]);
    for (int64_t n = 0; n < N; ++n) {
        if (!std::isfinite(dispersion[n]) || !(dispersion[n] > 0.0) || dispersion[n] > NB_ALPHA_MAX)
            return fail("dispersion must be finite and in (0, %g]: sample %lld holds %g", NB_ALPHA_MAX, (long long)n, dispersion[n]);
        double mean = 0.0;
        for (int v = 0; v < V; ++v)
            for (int k = 0; k < K; ++k) mean += exposures[(size_t)n * K + k] * signatures[(size_t)k * V + v];
        if (!(mean <= NB_MAX_MEAN)) return fail("the model's row sums must not exceed 2^24: row %lld sums to %g", (long long)n, mean);
    }
    std::vector<double> gd, gc;
    nb_gamma_constants(dispersion, N, gd, gc);
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    const size_t NV = (size_t)N * V;
    const int chunk = (int)chunk_rows(0, sizeof(double) * NV, B);
    const unsigned zero = 0;
    unsigned failed = 0;
    DevBufs d;
    CK(d.own_stream());
    double* dH = upload(d, exposures, (size_t)N * K);
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dalpha = upload(d, dispersion, (size_t)N);
    double* dgd = upload(d, gd);
    double* dgc = upload(d, gc);
    unsigned* dfailed = upload(d, &zero, 1);
    double* dout = d.get<double>((size_t)chunk * NV);
    if (!dH || !dW || !dalpha || !dgd || !dgc || !dfailed || !dout) return fail("hipMalloc failed (%d draws of %lld x %d)", chunk, (long long)N, V);
    for (int first = 0; first < B; first += chunk) {
        const int count = std::min(chunk, B - first);
        nb_launch_draw(dH, dW, dalpha, dgd, dgc, dout, dfailed, N, V, K, seed, 0.0, first, count, d.stream);
        HIPCK(hipGetLastError());
        CK(download(d, out + (size_t)first * NV, dout, (size_t)count * NV));
    }
    CK(download(d, &failed, dfailed, 1));
    HIPCK(hipStreamSynchronize(d.stream));
    *n_failed = (int)std::min<unsigned>(failed, 0x7fffffffu);
    return 0;
}

extern "C" int salnmf_nb_goodness_of_fit(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                         const double* dispersion, int n_draws, uint64_t seed, int min_iterations, int max_iterations, int conv_test_freq,
                                         double tol, int64_t chunk_bytes, double* exposures, double* errors, int* n_iterations, int* converged,
                                         int* n_exceed, double* null_mean, double* null_errors, int* null_n_iterations, double* draws, double* timings,
                                         int* n_failed) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, B = n_draws;
    if (!counts || !signatures || !dispersion || !exposures || !errors || !n_iterations || !converged || !n_exceed || !null_mean || !null_errors ||
        !null_n_iterations || !n_failed)
        return fail("null argument");
    CK(nb_check_draws(B));
    std::vector<double> x;
    CK(nb_check(counts, N, V, signatures, K, dispersion, min_iterations, max_iterations, conv_test_freq, tol, x));
    for (int64_t n = 0; n < N; ++n) {
        double total = 0.0;
        for (int v = 0; v < V; ++v) {
            const double c = counts[(size_t)n * V + v];
            if (c != std::floor(c)) return fail("counts must be integers: row %lld, column %d holds %g", (long long)n, v, c);
            total += c;
        }
        if (total > NB_MAX_MEAN) return fail("row totals must not exceed 2^24: row %lld sums to %.0f", (long long)n, total);
    }
    std::vector<double> gd, gc;
    nb_gamma_constants(dispersion, N, gd, gc);
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    const int cus = prop.multiProcessorCount;
    const size_t NV = (size_t)N * V, NK = (size_t)N * K, NB = (size_t)N * B;

    // draws per chunk: the [chunk][N][V] buffer stays within chunk_bytes (at least one draw); a draw of sample n carries sample n's
    // dispersion, so a chunk's problems read the samples' dispersions repeated `chunk` times
    const int chunk = (int)chunk_rows(chunk_bytes, sizeof(double) * NV, B);
    std::vector<double> alpha((size_t)N * (size_t)chunk);
    for (size_t i = 0; i < alpha.size(); ++i) alpha[i] = dispersion[i % (size_t)N];
    const unsigned zero = 0;
    unsigned failed = 0;

    DevBufs d;
    CK(d.own_stream());
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dX = upload(d, x);
    double* dalpha = upload(d, alpha);
    double* dgd = upload(d, gd);
    double* dgc = upload(d, gc);
    unsigned* dfailed = upload(d, &zero, 1);
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
    if (!dW || !dX || !dalpha || !dgd || !dgc || !dfailed || !dH || !derr || !dnit || !dconv || !dnext || !dXb || !dHb || !derr_b || !dnit_b || !dconv_b ||
        !dexceed || !dmean)
        return fail("hipMalloc failed (%d draws of %lld x %d, %d signatures)", B, (long long)N, V, K);

    Spans sp;  // draw, refit, reduce
    sp.start(d, timings != nullptr);
    const NbRefitArgs a{dX, dW, dalpha, dH, derr, dnit, dconv, dnext, N, V, K, min_iterations, max_iterations, conv_test_freq, tol};
    CK(sp.timed(1, [&] { return launch_nb_refit(a, cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < B; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, B - first);
        // from the device-resident exposures of the observed refit
        CK(sp.timed(0, [&]() -> int {
            nb_launch_draw(dH, dW, dalpha, dgd, dgc, dXb, dfailed, N, V, K, seed, SALNMF_EPSILON, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (draws) CK(download(d, draws + (size_t)first * NV, dXb, (size_t)count * NV));
        NbRefitArgs c = a;
        c.X = dXb;
        c.P = (int64_t)count * N;
        c.H = dHb;
        c.err = derr_b + (size_t)first * N;
        c.nit = dnit_b + (size_t)first * N;
        c.conv = dconv_b;
        CK(sp.timed(1, [&] { return launch_nb_refit(c, cus, d.stream); }));
    }
    const GofReduceArgs red{derr, derr_b, dexceed, dmean, N, B};
    CK(sp.timed(2, [&]() -> int {
        gof_launch_reduce(red, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    CK(download(d, exposures, dH, NK));
    CK(download(d, errors, derr, (size_t)N));
    CK(download(d, n_iterations, dnit, (size_t)N));
    CK(download(d, converged, dconv, (size_t)N));
    CK(download(d, n_exceed, dexceed, (size_t)N));
    CK(download(d, null_mean, dmean, (size_t)N));
    CK(download(d, null_errors, derr_b, NB));
    CK(download(d, null_n_iterations, dnit_b, NB));
    CK(download(d, &failed, dfailed, 1));
    HIPCK(hipStreamSynchronize(d.stream));
    if (draws)  // plain counts: the clipped zeros restored to 0
        for (size_t i = 0; i < (size_t)B * NV; ++i)
            if (draws[i] < 1.0) draws[i] = 0.0;
    CK(sp.totals(3, timings));
    if (timings) timings[3] = (double)n_chunks;
    *n_failed = (int)std::min<unsigned>(failed, 0x7fffffffu);
    return 0;
}
