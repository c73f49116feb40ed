// Host side of the negative-binomial refit (include/salnmf.h: salnmf_nb_refit_exposures) and the instantiations of its kernel
// (salnmf_nb.h: nb_refit_kernel); and of the draw from the fitted negative-binomial model and the
// goodness-of-fit test on it (salnmf_draw_nb_counts, salnmf_nb_goodness_of_fit).  A translation unit of its
// own, as section 20's: the tile-solve kernels of salnmf_refit.hip fill the register file, and nothing added here can move their
// allocation.  The three entry points are their Poisson counterparts' drivers (salnmf_refit_drivers.h: bootstrap_refit, gof_run,
// draw_run) with NbRefitArgs, this unit's launcher and nb_launch_draw: each checks its arguments (salnmf_host_kit.h, and the
// dispersions here), uploads the model's own arrays and makes one call.  The kernels behind the drivers are other units':
// resample_counts_kernel, nb_draw_kernel and gof_reduce_kernel in salnmf_batch.hip, refit_reduce_kernel in salnmf_refit.hip.
#define SALNMF_TEMPLATES_ONLY 1
#define SALNMF_REFIT_KERNELS 1
#define SALNMF_NB_KERNELS 1
#include "../../include/salnmf.h"
#include "salnmf_kernels.h"
#include "salnmf_device.h"
#include "salnmf_refit_drivers.h"
#include "salnmf_nb.h"
#include "salnmf_nbdraw.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

using namespace salnmf;

namespace {

int launch_nb_refit(const NbRefitArgs& a, int cus, hipStream_t stream) {
    return launch_tiles("negative-binomial refit", a.P, a.K, a.next_tile, cus, stream,
                        [&](auto kt, dim3 grid) { hipLaunchKernelGGL(nb_refit_kernel<decltype(kt)::value>, grid, dim3(BLOCK), 0, stream, a); });
}

// A problem list of `copies` resamples (draws) of the samples reads the samples' dispersions repeated `copies` times: a copy of
// sample n carries sample n's dispersion
std::vector<double> nb_tile_dispersion(const double* dispersion, int64_t N, int copies) {
    std::vector<double> alpha((size_t)N * (size_t)copies);
    for (size_t i = 0; i < alpha.size(); ++i) alpha[i] = dispersion[i % (size_t)N];
    return alpha;
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
    CK(check_refit_ranges(N, V, K, R, min_iterations, max_iterations, conv_test_freq, tol, Q,
                          exposures_mean && n_iterations_resampled && errors_resampled && (Q <= 0 || (quantiles && exposures_quantiles))));
    CK(nb_check_dispersion(dispersion, N));
    CK(check_signatures(signatures, K, V));
    std::vector<double> x;
    CK(clip_counts(counts, N, V, x));
    std::vector<uint32_t> icounts;
    RefitReduceArgs red{};
    if (R > 0) CK(check_resamples(counts, N, V, R, Q, quantiles, icounts, red.index));
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    const int chunk = bootstrap_chunk(chunk_bytes, N, V, R);
    const std::vector<double> alpha = nb_tile_dispersion(dispersion, N, std::max(chunk, 1));

    // (host buffers of the asynchronous copies live until d's destructor has waited for the stream)
    DevBufs d;
    CK(d.own_stream());
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dX = upload(d, x);
    double* dalpha = upload(d, alpha);
    const NbRefitArgs a{dX, dW, dalpha, nullptr, nullptr, nullptr, nullptr, nullptr, N, V, K, min_iterations, max_iterations, conv_test_freq, tol};
    const BootstrapRun io{R, Q, chunk, seed, icounts, red, prop.multiProcessorCount, exposures, errors, n_iterations, converged,
                          exposures_quantiles, exposures_mean, n_iterations_resampled, errors_resampled, exposures_resampled, timings};
    return bootstrap_refit(d, "negative-binomial refit", dW && dX && dalpha, a, io, launch_nb_refit);
}

// ---- draws from the fitted negative-binomial model and the goodness-of-fit test on them (salnmf_nbdraw.h)

extern "C" int salnmf_draw_nb_counts(int device, const double* exposures, int64_t n_samples, int n_signatures, const double* signatures, int n_features,
                                     const double* dispersion, int n_draws, uint64_t seed, double* out, int* n_failed) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, B = n_draws;
    if (!exposures || !signatures || !dispersion || !out || !n_failed) return fail("null argument");
    CK(check_model_draw(exposures, N, K, signatures, V, B));
    CK(nb_check_dispersion(dispersion, N));
    for (int64_t n = 0; n < N; ++n) {
        const double mean = nb_model_row_sum(exposures + (size_t)n * K, signatures, K, V);
        if (!(mean <= NB_MAX_MEAN)) return fail("the model's row sums must not exceed 2^24: row %lld sums to %g", (long long)n, mean);
    }
    std::vector<double> gd, gc;
    nb_gamma_constants(dispersion, N, gd, gc);
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
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
    CK(draw_run(d, dH && dW && dalpha && dgd && dgc && dfailed, N, V, B, out, [&](double* dout, int first, int count) {
        nb_launch_draw(dH, dW, dalpha, dgd, dgc, dout, dfailed, N, V, K, seed, 0.0, first, count, d.stream);
    }));
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
    CK(check_n_draws(B));
    CK(check_refit_ranges(N, V, K, 0, min_iterations, max_iterations, conv_test_freq, tol, 0, true));
    CK(nb_check_dispersion(dispersion, N));
    CK(check_signatures(signatures, K, V));
    std::vector<double> x;
    CK(clip_counts(counts, N, V, x));
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
    const int chunk = (int)chunk_rows(chunk_bytes, sizeof(double) * (size_t)N * V, B);
    const std::vector<double> alpha = nb_tile_dispersion(dispersion, N, chunk);
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
    const NbRefitArgs a{dX, dW, dalpha, nullptr, nullptr, nullptr, nullptr, nullptr, N, V, K, min_iterations, max_iterations, conv_test_freq, tol};
    const GofRun io{B, chunk, prop.multiProcessorCount, exposures, errors, n_iterations, converged, n_exceed, null_mean, null_errors, null_n_iterations,
                    draws, timings};
    CK(gof_run(
        d, dW && dX && dalpha && dgd && dgc && dfailed, a, io, launch_nb_refit,
        [&](const double* dH, double* dXb, int first, int count) {
            nb_launch_draw(dH, dW, dalpha, dgd, dgc, dXb, dfailed, N, V, K, seed, SALNMF_EPSILON, first, count, d.stream);
        },
        [&] { return download(d, &failed, dfailed, 1); }));
    *n_failed = (int)std::min<unsigned>(failed, 0x7fffffffu);
    return 0;
}
