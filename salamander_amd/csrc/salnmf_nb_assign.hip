// Host side of the sparse assignment under the negative-binomial likelihood (include/salnmf.h: salnmf_nb_assign_signatures) and
// the instantiations of its kernel (salnmf_nb_assign.h: nb_assign_kernel), DESIGN.md section 25.  A translation unit of its own, as
// salnmf_nb.hip is: the tile-solve kernels of salnmf_refit.hip and salnmf_nb.hip fill the register file, and nothing added here can
// move their allocation.  The entry point is salnmf_assign_signatures_ex's driver (salnmf_refit_drivers.h: assign_check,
// refit_prepare, assign_run) with NbAssignArgs and this unit's launcher: it checks its arguments (the dispersions where
// salnmf_nb_refit_exposures checks them), uploads W, the clipped counts and the dispersions, and makes one call.  The kernels
// behind the driver are other units': resample_counts_kernel in salnmf_batch.hip, refit_reduce_kernel and assign_selection_kernel
// in salnmf_refit.hip.
#define SALNMF_TEMPLATES_ONLY 1
#define SALNMF_REFIT_KERNELS 1
#define SALNMF_NB_KERNELS 1
#define SALNMF_NB_PIECES_ONLY 1
#include "../../include/salnmf.h"
#include "salnmf_kernels.h"
#include "salnmf_device.h"
#include "salnmf_refit_drivers.h"
#include "salnmf_nb_assign.h"

#include <cstdint>

using namespace salnmf;

namespace {

int launch_nb_assign(const NbAssignArgs& a, int cus, hipStream_t stream) {
    return launch_tiles("negative-binomial assignment", a.P, a.K, a.next_tile, cus, stream,
                        [&](auto kt, dim3 grid) { hipLaunchKernelGGL(nb_assign_kernel<decltype(kt)::value>, grid, dim3(BLOCK), 0, stream, a); });
}

}  // namespace

extern "C" int salnmf_nb_assign_signatures(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                           const double* dispersion, int n_resamples, uint64_t seed, int n_quantiles, const double* quantiles,
                                           int min_iterations, int max_iterations, int conv_test_freq, double tol, double max_kl_increase,
                                           int64_t chunk_bytes, const uint8_t* candidates, const uint8_t* required, int readd, double* exposures, int* active,
                                           double* errors, int* removal_round, double* kl_increase, int* n_trials, int64_t* n_iterations, int* converged,
                                           double* dense_exposures, double* dense_errors, int* dense_n_iterations, int* dense_converged,
                                           double* selection_frequency, double* exposures_quantiles, double* exposures_mean, double* exposures_resampled,
                                           int* readd_round, double* kl_decrease, double* timings) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, R = n_resamples, Q = n_quantiles;
    const AssignOutputs out{exposures, active, errors, removal_round, kl_increase, n_trials, n_iterations, converged, dense_exposures, dense_errors,
                            dense_n_iterations, dense_converged, selection_frequency, exposures_quantiles, exposures_mean, exposures_resampled, readd_round,
                            kl_decrease, timings};
    CK(assign_check(out, counts && signatures && dispersion, readd, max_kl_increase, max_iterations, conv_test_freq));
    RefitInputs in;
    CK(refit_prepare(device, counts, N, V, signatures, K, R, Q, quantiles, min_iterations, max_iterations, conv_test_freq, tol,
                     selection_frequency && exposures_mean && (Q <= 0 || (quantiles && exposures_quantiles)), in, AssignSets{candidates, required, readd},
                     [&] { return nb_check_dispersion(dispersion, N); }));
    // (host buffers of the asynchronous copies live until d's destructor has waited for the stream)
    DevBufs d;
    CK(d.own_stream());
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dX = upload(d, in.x);
    double* dalpha = upload(d, dispersion, (size_t)N);  // (not tiled: problem p reads alpha[p % N])
    NbAssignArgs a{};
    a.X = dX, a.W = dW, a.alpha = dalpha, a.P = N, a.V = V, a.K = K;
    a.min_it = min_iterations, a.max_it = max_iterations, a.freq = conv_test_freq, a.tol = tol, a.thr = max_kl_increase, a.readd = readd;
    return assign_run(d, dW && dX && dalpha, a, in, R, Q, seed, chunk_bytes, out, launch_nb_assign);
}
