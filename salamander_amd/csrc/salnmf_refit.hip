// Host side of the refit to fixed signatures (include/salnmf.h: salnmf_refit_exposures) and its two kernels
// (salnmf_refit.h: refit_kernel, refit_reduce_kernel); and of the sparse assignment built on it
// (salnmf_assign_signatures, salnmf_assign_signatures_ex; salnmf_assign.h: assign_kernel, assign_selection_kernel), DESIGN.md sections 14
// and 14.1; and of the goodness-of-fit test built on it (salnmf_draw_model_counts, salnmf_goodness_of_fit; salnmf_gof.h:
// model_draw_kernel, gof_reduce_kernel, which salnmf_batch.hip compiles); and of the signature-presence test
// (salnmf_signature_presence; salnmf_presence.h: presence_kernel here, presence_draw_kernel in salnmf_batch.hip), DESIGN.md section 17;
// and of that test's power analysis (salnmf_signature_power; salnmf_power.h: its three kernels in salnmf_batch.hip), DESIGN.md section 18;
// and of the profile likelihood of one exposure and its interval (salnmf_profile_likelihood, salnmf_exposure_intervals;
// salnmf_profile.h: profile_kernel); and of the test of changed exposure shares between two samples
// (salnmf_exposure_change; salnmf_change.h: change_kernel here, change_draw_kernel in salnmf_batch.hip); and of
// the per-signature test of a changed share (salnmf_signature_change; salnmf_sigchange.h: sigchange_kernel here, sigchange_draw_kernel in
// salnmf_batch.hip), DESIGN.md section 22.  The six tile-solve kernels share the solve_* pieces of salnmf_refit.h; the drivers below share one kit:
// from salnmf_host_kit.h launch_tiles, the argument checks, Spans, chunk_rows and upload / download; from salnmf_refit_drivers.h
// refit_prepare, bootstrap_refit, gof_run, draw_run and assign_run, which the negative-binomial entry points of salnmf_nb.hip and
// salnmf_nb_assign.hip call too; refit_launch_reduce and assign_launch_selection here, next to their kernels; and for the pair calls pair_observed and pair_draw_solve.
#define SALNMF_TEMPLATES_ONLY 1
#define SALNMF_REFIT_KERNELS 1
#define SALNMF_REFIT_REDUCE_KERNEL 1
#define SALNMF_ASSIGN_SELECT_KERNEL 1
#include "../../include/salnmf.h"
#include "salnmf_kernels.h"
#include "salnmf_device.h"
#include "salnmf_refit_drivers.h"
#include "salnmf_assign.h"
#include "salnmf_gof.h"
#include "salnmf_presence.h"
#include "salnmf_change.h"
#include "salnmf_sigchange.h"
#include "salnmf_power.h"
#include "salnmf_profile.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <type_traits>
#include <vector>

using namespace salnmf;

namespace {

// ---- the launchers of the tile-solve kernels (salnmf_host_kit.h: launch_tiles)

int launch_refit(const RefitArgs& a, int cus, hipStream_t stream) {
    return launch_tiles("refit", a.P, a.K, a.next_tile, cus, stream,
                        [&](auto kt, dim3 grid) { hipLaunchKernelGGL(refit_kernel<decltype(kt)::value>, grid, dim3(BLOCK), 0, stream, a); });
}

int launch_assign(const AssignArgs& a, int cus, hipStream_t stream) {
    // candidate sets, required signatures and the re-addition pass have instantiations of their own
    const bool ex = a.cand || a.req || a.readd;
    return launch_tiles("assignment", a.P, a.K, a.next_tile, cus, stream, [&](auto kt, dim3 grid) {
        if (ex) hipLaunchKernelGGL((assign_kernel<decltype(kt)::value, true>), grid, dim3(BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((assign_kernel<decltype(kt)::value, false>), grid, dim3(BLOCK), 0, stream, a);
    });
}

int launch_presence(const PresenceArgs& a, int cus, hipStream_t stream) {
    return launch_tiles("presence", a.P, a.K, a.next_tile, cus, stream,
                        [&](auto kt, dim3 grid) { hipLaunchKernelGGL(presence_kernel<decltype(kt)::value>, grid, dim3(BLOCK), 0, stream, a); });
}

int launch_profile(const ProfileArgs& a, int cus, hipStream_t stream) {
    return launch_tiles("profile", a.P, a.K, a.next_tile, cus, stream,
                        [&](auto kt, dim3 grid) { hipLaunchKernelGGL(profile_kernel<decltype(kt)::value>, grid, dim3(BLOCK), 0, stream, a); });
}

}  // namespace

void salnmf::refit_launch_reduce(RefitReduceArgs& red, const double* H, double* quant, double* mean, int64_t N, int K, int R, int Q, hipStream_t stream) {
    red.H = H, red.quant = quant, red.mean = mean;
    red.N = N, red.K = K, red.R = R, red.Q = Q;
    red.R2 = 1;
    while (red.R2 < R) red.R2 <<= 1;
    hipLaunchKernelGGL(refit_reduce_kernel, dim3((unsigned)N), dim3(REFIT_SORT_BLOCK), 0, stream, red);
}

void salnmf::assign_launch_selection(const double* H, double* freq, int64_t NK, int R, hipStream_t stream) {
    const AssignSelectArgs sel{H, freq, NK, R};
    hipLaunchKernelGGL(assign_selection_kernel, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, stream, sel);
}

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
    // (host buffers of the asynchronous copies live until d's destructor has waited for the stream)
    DevBufs d;
    CK(d.own_stream());
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dX = upload(d, in.x);
    const RefitArgs a{dX, dW, nullptr, nullptr, nullptr, nullptr, nullptr, N, V, K, min_iterations, max_iterations, conv_test_freq, tol};
    const BootstrapRun io{R, Q, bootstrap_chunk(chunk_bytes, N, V, R), seed, in.icounts, in.red, in.cus, exposures, errors, n_iterations, converged,
                          exposures_quantiles, exposures_mean, n_iterations_resampled, errors_resampled, exposures_resampled, timings};
    return bootstrap_refit(d, "refit", dW && dX, a, io, launch_refit);
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
    const AssignOutputs out{exposures, active, errors, removal_round, kl_increase, n_trials, n_iterations, converged, dense_exposures, dense_errors,
                            dense_n_iterations, dense_converged, selection_frequency, exposures_quantiles, exposures_mean, exposures_resampled, readd_round,
                            kl_decrease, timings};
    CK(assign_check(out, counts && signatures, readd, max_kl_increase, max_iterations, conv_test_freq));
    RefitInputs in;
    CK(refit_prepare(device, counts, N, V, signatures, K, R, Q, quantiles, min_iterations, max_iterations, conv_test_freq, tol,
                     selection_frequency && exposures_mean && (Q <= 0 || (quantiles && exposures_quantiles)), in, AssignSets{candidates, required, readd}));
    DevBufs d;
    CK(d.own_stream());
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dX = upload(d, in.x);
    AssignArgs a{};
    a.X = dX, a.W = dW, a.P = N, a.V = V, a.K = K;
    a.min_it = min_iterations, a.max_it = max_iterations, a.freq = conv_test_freq, a.tol = tol, a.thr = max_kl_increase, a.readd = readd;
    return assign_run(d, dW && dX, a, in, R, Q, seed, chunk_bytes, out, launch_assign);
}

// ---- goodness of fit by parametric bootstrap (salnmf_gof.h)

extern "C" int salnmf_draw_model_counts(int device, const double* exposures, int64_t n_samples, int n_signatures, const double* signatures,
                                        int n_features, const double* totals, int n_draws, uint64_t seed, double* out) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, B = n_draws;
    if (!exposures || !signatures || !totals || !out) return fail("null argument");
    CK(check_model_draw(exposures, N, K, signatures, V, B));
    std::vector<uint32_t> trials((size_t)N);
    for (int64_t n = 0; n < N; ++n) {
        const double t = totals[n];
        if (!(t >= 0.0) || t >= 4294967296.0 || t != (double)(uint64_t)t)
            return fail("totals must be non-negative integers below 2^32: row %lld holds %g", (long long)n, t);
        trials[(size_t)n] = (uint32_t)t;
    }
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    DevBufs d;
    CK(d.own_stream());
    double* dH = upload(d, exposures, (size_t)N * K);
    double* dW = upload(d, signatures, (size_t)K * V);
    uint32_t* dT = upload(d, trials);
    CK(draw_run(d, dH && dW && dT, N, V, B, out, [&](double* dout, int first, int count) {
        gof_launch_model_draw(dH, dW, dT, nullptr, dout, N, V, K, seed, 0.0, first, count, d.stream);
    }));
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
    CK(check_n_draws(B));
    RefitInputs in;
    CK(refit_prepare(device, counts, N, V, signatures, K, 0, 0, nullptr, min_iterations, max_iterations, conv_test_freq, tol, true, in));
    CK(refit_check_counts(counts, N, V, in.icounts));  // integer counts, row totals below 2^32 (the values themselves are not used)

    DevBufs d;
    CK(d.own_stream());
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dX = upload(d, in.x);
    const RefitArgs a{dX, dW, nullptr, nullptr, nullptr, nullptr, nullptr, N, V, K, min_iterations, max_iterations, conv_test_freq, tol};
    const GofRun io{B, (int)chunk_rows(chunk_bytes, sizeof(double) * (size_t)N * V, B), in.cus, exposures, errors, n_iterations, converged, n_exceed,
                    null_mean, null_errors, null_n_iterations, draws, timings};
    return gof_run(
        d, dW && dX, a, io, launch_refit,
        [&](const double* dH, double* dXb, int first, int count) {  // a row's trial count is read off the clipped counts
            gof_launch_model_draw(dH, dW, nullptr, dX, dXb, N, V, K, seed, SALNMF_EPSILON, first, count, d.stream);
        },
        [] { return 0; });  // (no download of its own)
}

// ---- the pair run: what the presence test (salnmf_presence.h), its power analysis (salnmf_power.h, section
// 18) and the profile likelihood with its intervals (salnmf_profile.h, section 19) do alike.  All four entry points run
// pair_observed; the first two go on with their draws (presence_enqueue, pair_draw_solve) and presence_finish, the power
// analysis putting its launches on the same stream in between; the last two wait (profile_observed), list their problems on
// the host, run one profile_kernel launch and scatter its trials.  The shared part is salnmf_refit_drivers.h's pair run, which
// salnmf_nb_presence.hip instantiates with the negative-binomial model; here it runs with the Poisson one.

namespace {

// The Poisson model of the pair run (salnmf_refit_drivers.h): no inputs of its own, presence_kernel, and the conditional model
// draw of salnmf_presence.h from the device-resident null fits (a row's trial count is read off the clipped counts)
struct PoissonPresence {
    int own_checks() const { return 0; }
    bool inputs(DevBufs&, PresenceArgs&) const { return true; }
    int launch(const PresenceArgs& a, int cus, hipStream_t stream) const { return launch_presence(a, cus, stream); }
    int after_observed(const PairIO&, PairRunOf<PresenceArgs>&) const { return 0; }
    void draw(PairRunOf<PresenceArgs>& r, uint64_t seed, int first, int count) const {
        presence_launch_draw(r.dH0, r.dW, r.dX, r.dpn, r.dps, r.dXb, (int64_t)r.NP, r.a.V, r.a.K, seed, SALNMF_EPSILON, first, count, r.d->stream);
    }
    int before_wait(DevBufs&) const { return 0; }
};

struct PairRun : PairRunOf<PresenceArgs> {
    int launch_profile_kernel(const PairIO& io, ProfileArgs pa) {
        pa.X = dX, pa.W = dW, pa.cand = dcand, pa.next_tile = a.next_tile;
        pa.V = io.V, pa.K = io.K, pa.min_it = io.min_iterations, pa.max_it = io.max_iterations, pa.freq = io.conv_test_freq, pa.tol = io.tol;
        return sp.timed(1, [&] { return launch_profile(pa, in.cus, d->stream); });
    }
    // (after the stream has been waited for)
    int profile_times(const PairIO& io, int64_t P) {
        CK(sp.totals(2, io.timings));
        if (io.timings) io.timings[2] = (double)P;
        return 0;
    }
};

// The profile calls' start: pair_observed (the counts need not be integers: nothing is drawn), waited for, and the alternative
// fit scattered.
int profile_observed(const PairIO& io, PairRun& r) {
    if (!io.counts || !io.signatures || !io.test || !io.tested || !io.exposures || !io.errors) return fail("null argument");
    PoissonPresence m;
    CK(pair_observed(io, false, 0, r, m));
    if (io.timings) io.timings[0] = io.timings[1] = io.timings[2] = 0.0;
    if (r.NP == 0) return 0;
    HIPCK(hipStreamSynchronize(r.d->stream));
    pair_scatter_alternative(io, r);
    return 0;
}

}  // namespace

extern "C" int salnmf_signature_presence(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                         const int* test, int n_test, const uint8_t* candidates, int n_draws, uint64_t seed, int min_iterations,
                                         int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes, uint8_t* tested, double* statistic,
                                         int* n_exceed, double* null_mean, double* exposures, double* errors, double* null_exposures, double* null_errors,
                                         int* n_iterations, int* converged, double* null_statistics, int* null_n_iterations, double* draws,
                                         double* timings) {
    const PairIO io{device, counts, n_samples, n_features, signatures, n_signatures, test, n_test, candidates, min_iterations, max_iterations,
                    conv_test_freq, tol, tested, exposures, errors, timings, n_draws, seed, chunk_bytes, statistic, n_exceed, null_mean, null_exposures,
                    null_errors, n_iterations, converged, null_statistics, null_n_iterations, draws};
    PoissonPresence m;
    PairRun r;
    CK(presence_enqueue(io, 0, r, m));
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
    CK(check_n_draws(B));
    if (L < 1 || L > POWER_MAX_SHARES) return fail("n_shares must be in [1, %d], got %d", POWER_MAX_SHARES, L);
    for (int l = 0; l < L; ++l) {
        if (!std::isfinite(shares[l]) || shares[l] < 0.0 || shares[l] >= 1.0) return fail("share %d must be finite and in [0, 1), got %g", l, shares[l]);
        if (l > 0 && !(shares[l] > shares[l - 1])) return fail("shares must be strictly ascending: share %d is %g after %g", l, shares[l], shares[l - 1]);
    }
    if (A < 1 || A > POWER_MAX_DRAWS) return fail("n_alt_draws must be in [1, %d], got %d", POWER_MAX_DRAWS, A);
    if (max_exceed < 0 || max_exceed > B) return fail("max_exceed must be in [0, %d], got %d", B, max_exceed);
    const int64_t R = (int64_t)L * A;  // rows r = l A + a
    const PairIO io{device, counts, n_samples, n_features, signatures, n_signatures, test, n_test, candidates, min_iterations, max_iterations,
                    conv_test_freq, tol, tested, exposures, errors, timings, n_draws, seed, chunk_bytes, statistic, n_exceed, null_mean, null_exposures,
                    null_errors, n_iterations, converged, null_statistics, null_n_iterations, draws};
    std::vector<double> h_Hp, h_stat_a, h_mean_a, h_draws_a;  // (before r: they outlive the copies into them, which r.d waits for)
    std::vector<int> h_nit_a, h_exceed_a, h_ndet;
    PoissonPresence m;
    PairRun r;
    CK(presence_enqueue(io, R, r, m));
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
    double* dshares = upload(d, shares, (size_t)L);
    double* dHp = d.get<double>((size_t)L * PK);
    double* dstat_a = d.get<double>((size_t)R * NP);
    int* dnit_a = d.get<int>(2 * (size_t)R * NP);
    int* dexceed_a = d.get<int>((size_t)R * NP);
    int* dndet = d.get<int>((size_t)L * NP);
    double* dmean_a = d.get<double>((size_t)L * NP);
    if (!dshares || !dHp || !dstat_a || !dnit_a || !dexceed_a || !dndet || !dmean_a)
        return fail("hipMalloc or upload failed (%d shares x %d draws of %zu pairs x %d, %d signatures)", L, A, NP, V, K);
    CK(r.sp.timed(3, [&]() -> int {
        power_launch_plant(PowerPlantArgs{r.dH0, r.dps, dshares, dHp, (int64_t)NP, K, L}, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    // rows per chunk: the presence test's buffer and rule
    int n_chunks = 0;
    CK(pair_draw_solve(r, m, R, std::min<int64_t>(R, r.chunk_rows), [&](int64_t first, int64_t count) {
        power_launch_draw(dHp, r.dW, r.dX, r.dpn, r.dps, r.dXb, (int64_t)NP, V, K, seed, SALNMF_EPSILON, A, first, count, d.stream);
    }, dstat_a, dnit_a, alt_draws ? h_draws_a.data() : nullptr, 4, 5, &n_chunks));
    CK(r.sp.timed(6, [&]() -> int {
        power_launch_reduce(PowerReduceArgs{r.dstat_b, dstat_a, dexceed_a, dndet, dmean_a, (int64_t)NP, B, L, A, max_exceed}, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    CK(download(d, h_Hp.data(), dHp, h_Hp.size()));
    CK(download(d, h_stat_a.data(), dstat_a, h_stat_a.size()));
    CK(download(d, h_nit_a.data(), dnit_a, h_nit_a.size()));
    CK(download(d, h_exceed_a.data(), dexceed_a, h_exceed_a.size()));
    CK(download(d, h_ndet.data(), dndet, h_ndet.size()));
    CK(download(d, h_mean_a.data(), dmean_a, h_mean_a.size()));
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
        for (int i = 3; i < 7; ++i) CK(r.sp.total_ms(i, timings + i + 1));
        timings[8] = (double)n_chunks;
    }
    return 0;
}

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
    const PairIO io{device, counts, N, n_features, signatures, K, test, S, candidates, min_iterations, max_iterations, conv_test_freq, tol, tested,
                    exposures, errors, timings, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // (before r: they outlive the copies into and out of them, which r.d waits for)
    std::vector<int> prob_n, prob_s, count, h_nit, h_conv;
    std::vector<double> vals, h_f, h_H;
    PairRun r;
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
    a.prob_n = upload(d, prob_n), a.prob_s = upload(d, prob_s), a.count = upload(d, count), a.values = upload(d, vals);
    a.trial_f = d.get<double>(P * T), a.trial_nit = d.get<int>(P * T), a.trial_conv = d.get<int>(P * T);
    a.trial_H = profile_exposures ? d.get<double>(P * T * K) : nullptr;
    if (!a.prob_n || !a.prob_s || !a.count || !a.values || !a.trial_f || !a.trial_nit || !a.trial_conv || (profile_exposures && !a.trial_H))
        return fail("hipMalloc or upload failed (%zu problems of %d values, %d signatures)", P, T, K);
    a.P = (int64_t)P, a.T = T;
    CK(r.launch_profile_kernel(io, a));
    CK(download(d, h_f.data(), a.trial_f, h_f.size()));
    CK(download(d, h_nit.data(), a.trial_nit, h_nit.size()));
    CK(download(d, h_conv.data(), a.trial_conv, h_conv.size()));
    if (a.trial_H) CK(download(d, h_H.data(), a.trial_H, h_H.size()));
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
    return r.profile_times(io, (int64_t)P);
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
    const PairIO io{device, counts, N, n_features, signatures, K, test, S, candidates, min_iterations, max_iterations, conv_test_freq, tol, tested,
                    exposures, errors, timings, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<int> prob_n, prob_s, end, h_nt, h_br;
    std::vector<double> hhat, f1, h_c, h_f, h_lo, h_hi;
    std::vector<size_t> prob_pair;
    PairRun r;
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
    a.prob_n = upload(d, prob_n), a.prob_s = upload(d, prob_s), a.end = upload(d, end);
    a.hhat = upload(d, hhat), a.f1 = upload(d, f1);
    a.trial_c = d.get<double>(P * T), a.trial_f = d.get<double>(P * T), a.trial_nit = d.get<int>(P * T), a.trial_conv = d.get<int>(P * T);
    a.lo = d.get<double>(P), a.hi = d.get<double>(P), a.n_trials = d.get<int>(P), a.bracketed = d.get<int>(P);
    if (!a.prob_n || !a.prob_s || !a.end || !a.hhat || !a.f1 || !a.trial_c || !a.trial_f || !a.trial_nit || !a.trial_conv || !a.lo || !a.hi ||
        !a.n_trials || !a.bracketed)
        return fail("hipMalloc or upload failed (%zu problems of %d trials, %d signatures)", P, T, K);
    a.P = (int64_t)P, a.T = T, a.n_bisections = J, a.max_expansions = E, a.delta = delta;
    CK(r.launch_profile_kernel(io, a));
    CK(download(d, h_c.data(), a.trial_c, h_c.size()));
    CK(download(d, h_f.data(), a.trial_f, h_f.size()));
    CK(download(d, h_lo.data(), a.lo, P));
    CK(download(d, h_hi.data(), a.hi, P));
    CK(download(d, h_nt.data(), a.n_trials, P));
    CK(download(d, h_br.data(), a.bracketed, P));
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
    return r.profile_times(io, (int64_t)P);
}

// ---- have the exposure shares changed between two samples?  Three solves per pair and per null draw (salnmf_change.h, DESIGN.md
// section 21).  The driver is the goodness-of-fit test's on a compact pair list: the observed launch, per chunk a draw and a solve
// launch, gof_reduce_kernel over the pairs, the downloads -- one stream, nothing waited for in between.

namespace {

int launch_change(const ChangeArgs& a, int cus, hipStream_t stream) {
    return launch_tiles("change", a.P, a.K, a.next_tile, cus, stream,
                        [&](auto kt, dim3 grid) { hipLaunchKernelGGL(change_kernel<decltype(kt)::value>, grid, dim3(BLOCK), 0, stream, a); });
}

}  // namespace

extern "C" int salnmf_exposure_change(int device, const double* counts_a, int64_t n_samples, int n_features, const double* counts_b,
                                      int64_t n_samples_b, int n_features_b, const double* signatures, int n_signatures, const uint8_t* candidates,
                                      int n_draws, uint64_t seed, int min_iterations, int max_iterations, int conv_test_freq, double tol,
                                      int64_t chunk_bytes, uint8_t* tested, double* statistic, int* n_exceed, double* null_mean, double* exposures_a,
                                      double* exposures_b, double* pooled_exposures, double* errors, double* null_errors, int* n_iterations,
                                      int* converged, double* null_statistics, int* null_n_iterations, double* draws, double* timings) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, B = n_draws;
    if (!counts_a || !counts_b || !signatures || !tested || !statistic || !n_exceed || !null_mean || !exposures_a || !exposures_b || !pooled_exposures ||
        !errors || !null_errors || !n_iterations || !converged || !null_statistics || !null_n_iterations)
        return fail("null argument");
    if (n_samples_b != N || n_features_b != V)
        return fail("row n of counts_a and row n of counts_b form pair n: the shapes must agree, got %lld x %d and %lld x %d", (long long)N, V,
                    (long long)n_samples_b, n_features_b);
    CK(check_n_draws(B));
    if (conv_test_freq >= 1 && max_iterations >= 0 && max_iterations % conv_test_freq != 0)
        return fail("max_iterations must be a multiple of conv_test_freq, got %d and %d", max_iterations, conv_test_freq);
    // the host ends of the asynchronous copies live until d's destructor has waited for the stream: d is declared after them
    RefitInputs in, in_b;
    CK(refit_prepare(device, counts_a, N, V, signatures, K, 0, 0, nullptr, min_iterations, max_iterations, conv_test_freq, tol, true, in,
                     AssignSets{candidates, nullptr, 0}));
    CK(refit_prepare(device, counts_b, N, V, signatures, K, 0, 0, nullptr, min_iterations, max_iterations, conv_test_freq, tol, true, in_b));
    CK(refit_check_counts(counts_a, N, V, in.icounts));  // integer counts, row totals below 2^32
    CK(refit_check_counts(counts_b, N, V, in_b.icounts));
    const int cus = in.cus;

    // the tested pairs: at least two candidates and a positive total on either side
    const int words = ((K + 15) / 16 + 1) / 2;
    std::vector<int> pair_n;
    for (int64_t n = 0; n < N; ++n) {
        int size = K;
        if (candidates) {
            size = 0;
            for (int w = 0; w < words; ++w) size += __builtin_popcount(in.cand[(size_t)n * words + w]);
        }
        uint64_t total_a = 0, total_b = 0;
        for (int v = 0; v < V; ++v) total_a += in.icounts[(size_t)n * V + v], total_b += in_b.icounts[(size_t)n * V + v];
        tested[n] = size > 1 && total_a > 0 && total_b > 0;
        if (tested[n]) pair_n.push_back((int)n);
    }
    const size_t NP = pair_n.size();
    if (NP > 0x3fffffff) return fail("%zu tested pairs: at most 2^30 - 1", NP);  // (the draw's grid: two workgroups per pair)
    const double nan = std::nan("");
    const size_t NK = (size_t)N * K, NB = (size_t)N * B;
    std::fill(statistic, statistic + N, nan);
    std::fill(null_mean, null_mean + N, nan);
    std::fill(n_exceed, n_exceed + N, 0);
    std::fill(exposures_a, exposures_a + NK, nan);
    std::fill(exposures_b, exposures_b + NK, nan);
    std::fill(pooled_exposures, pooled_exposures + NK, nan);
    std::fill(errors, errors + 3 * (size_t)N, nan);
    std::fill(null_errors, null_errors + 2 * (size_t)N, nan);
    std::fill(n_iterations, n_iterations + 3 * (size_t)N, 0);
    std::fill(converged, converged + 3 * (size_t)N, 0);
    std::fill(null_statistics, null_statistics + NB, nan);
    std::fill(null_n_iterations, null_n_iterations + 3 * NB, 0);
    if (draws) std::fill(draws, draws + 2 * NB * V, 0.0);
    if (timings) timings[0] = timings[1] = timings[2] = timings[3] = 0.0;
    if (NP == 0) return 0;

    // draws per chunk: the [chunk][pairs][2][V] buffer stays within chunk_bytes (at least one draw)
    const size_t PV2 = NP * 2 * V, PK = NP * K, PB = NP * B;
    const int chunk = (int)chunk_rows(chunk_bytes, sizeof(double) * PV2, B);
    std::vector<double> h_stat(NP), h_f(5 * NP), h_Ha(PK), h_Hb(PK), h_H0(PK), h_mean(NP), h_stat_b(PB), h_draws(draws ? PB * 2 * V : 0);
    std::vector<int> h_nit(3 * NP), h_conv(3 * NP), h_exceed(NP), h_nit_b(3 * PB);

    DevBufs d;
    CK(d.own_stream());
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dXa = upload(d, in.x);
    double* dXb = upload(d, in_b.x);
    int* dpn = upload(d, pair_n);
    uint32_t* dcand = candidates ? upload(d, in.cand) : nullptr;
    double* dstat = d.get<double>(NP);
    double* df = d.get<double>(5 * NP);
    int* dnit = d.get<int>(3 * NP);
    int* dconv = d.get<int>(3 * NP);
    double* dHa = d.get<double>(PK);
    double* dHb = d.get<double>(PK);
    double* dH0 = d.get<double>(PK);
    unsigned* dnext = d.get<unsigned>(1);
    double* dXd = d.get<double>((size_t)chunk * PV2);
    double* dstat_b = d.get<double>(PB);
    int* dnit_b = d.get<int>(3 * PB);
    int* dexceed = d.get<int>(NP);
    double* dmean = d.get<double>(NP);
    if (!dW || !dXa || !dXb || !dpn || (candidates && !dcand) || !dstat || !df || !dnit || !dconv || !dHa || !dHb || !dH0 || !dnext || !dXd || !dstat_b ||
        !dnit_b || !dexceed || !dmean)
        return fail("hipMalloc or upload failed (%d draws of %zu pairs x 2 x %d, %d signatures)", B, NP, V, K);

    Spans sp;  // draw, solve, reduce
    sp.start(d, timings != nullptr);
    const ChangeArgs a{dXa, dXb, dW, dpn, dcand, dstat, dnit, df, dconv, dHa, dHb, dH0, dnext, (int64_t)NP, (int64_t)NP, (int64_t)V, V, K, 1,
                       min_iterations, max_iterations, conv_test_freq, tol};
    CK(sp.timed(1, [&] { return launch_change(a, cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < B; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, B - first);
        // from the device-resident exposures of the observed pooled fits; a side's trial count is read off its clipped counts
        CK(sp.timed(0, [&]() -> int {
            change_launch_draw(dH0, dW, dXa, dXb, dpn, dXd, (int64_t)NP, V, K, seed, SALNMF_EPSILON, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (draws) CK(download(d, h_draws.data() + (size_t)first * PV2, dXd, (size_t)count * PV2));
        ChangeArgs c = a;
        c.Xa = dXd, c.Xb = dXd + V, c.stride = 2 * (int64_t)V, c.by_sample = 0;
        c.P = (int64_t)count * (int64_t)NP;
        c.stat = dstat_b + (size_t)first * NP;
        c.nit = dnit_b + 3 * (size_t)first * NP;
        c.f = nullptr, c.conv = nullptr, c.Ha = nullptr, c.Hb = nullptr, c.H0 = nullptr;
        CK(sp.timed(1, [&] { return launch_change(c, cus, d.stream); }));
    }
    // gof_reduce_kernel over the pairs: n_exceed counts t_b >= t (false for a NaN on either side), null_mean sums from 0.0 in ascending b
    const GofReduceArgs red{dstat, dstat_b, dexceed, dmean, (int64_t)NP, B};
    CK(sp.timed(2, [&]() -> int {
        gof_launch_reduce(red, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    CK(download(d, h_stat, dstat));
    CK(download(d, h_f, df));
    CK(download(d, h_nit, dnit));
    CK(download(d, h_conv, dconv));
    CK(download(d, h_Ha, dHa));
    CK(download(d, h_Hb, dHb));
    CK(download(d, h_H0, dH0));
    CK(download(d, h_exceed, dexceed));
    CK(download(d, h_mean, dmean));
    CK(download(d, h_stat_b, dstat_b));
    CK(download(d, h_nit_b, dnit_b));
    HIPCK(hipStreamSynchronize(d.stream));

    // the compact pair list back into the (N, ...) results
    for (size_t j = 0; j < NP; ++j) {
        const size_t o = (size_t)pair_n[j];
        statistic[o] = h_stat[j];
        n_exceed[o] = h_exceed[j];
        null_mean[o] = h_mean[j];
        std::copy(h_Ha.begin() + j * K, h_Ha.begin() + (j + 1) * K, exposures_a + o * K);
        std::copy(h_Hb.begin() + j * K, h_Hb.begin() + (j + 1) * K, exposures_b + o * K);
        std::copy(h_H0.begin() + j * K, h_H0.begin() + (j + 1) * K, pooled_exposures + o * K);
        for (int i = 0; i < 3; ++i) errors[3 * o + i] = h_f[5 * j + i], n_iterations[3 * o + i] = h_nit[3 * j + i], converged[3 * o + i] = h_conv[3 * j + i];
        for (int i = 0; i < 2; ++i) null_errors[2 * o + i] = h_f[5 * j + 3 + i];
        for (size_t b = 0; b < (size_t)B; ++b) {
            null_statistics[b * N + o] = h_stat_b[b * NP + j];
            for (int i = 0; i < 3; ++i) null_n_iterations[3 * (b * N + o) + i] = h_nit_b[3 * (b * NP + j) + i];
            if (draws)  // plain counts: the clipped zeros restored to 0
                for (int i = 0; i < 2 * V; ++i) {
                    const double c = h_draws[(b * NP + j) * 2 * V + i];
                    draws[(b * N + o) * 2 * V + i] = c < 1.0 ? 0.0 : c;
                }
        }
    }
    CK(sp.totals(3, timings));
    if (timings) timings[3] = (double)n_chunks;
    return 0;
}

// ---- which signature's share has changed between two samples?  Two free solves and one tied solve per (pair, tested signature) and
// per null draw, a problem in two adjacent lane columns (salnmf_sigchange.h).  The driver is the change test's
// on the presence test's pair list: the observed launch, per chunk a draw and a solve launch, gof_reduce_kernel over the problems,
// the downloads -- one stream, nothing waited for in between.

namespace {

int launch_sigchange(const SigChangeArgs& a, int cus, hipStream_t stream) {
    // the tile list is of lane columns, two per problem
    return launch_tiles("signature change", 2 * a.P, a.K, a.next_tile, cus, stream,
                        [&](auto kt, dim3 grid) { hipLaunchKernelGGL(sigchange_kernel<decltype(kt)::value>, grid, dim3(BLOCK), 0, stream, a); });
}

}  // namespace

extern "C" int salnmf_signature_change(int device, const double* counts_a, int64_t n_samples, int n_features, const double* counts_b,
                                       int64_t n_samples_b, int n_features_b, const double* signatures, int n_signatures, const int* test, int n_test,
                                       const uint8_t* candidates, int n_draws, uint64_t seed, int min_iterations, int max_iterations,
                                       int conv_test_freq, double tol, int64_t chunk_bytes, uint8_t* tested, double* statistic, int* n_exceed,
                                       double* null_mean, double* exposures_a, double* exposures_b, double* tied_exposures_a, double* tied_exposures_b,
                                       double* errors, int* n_iterations, int* converged, double* null_statistics, int* null_n_iterations,
                                       double* draws, double* timings) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures, B = n_draws, S = n_test;
    if (!counts_a || !counts_b || !signatures || !test || !tested || !statistic || !n_exceed || !null_mean || !exposures_a || !exposures_b ||
        !tied_exposures_a || !tied_exposures_b || !errors || !n_iterations || !converged || !null_statistics || !null_n_iterations)
        return fail("null argument");
    if (n_samples_b != N || n_features_b != V)
        return fail("row n of counts_a and row n of counts_b form pair n: the shapes must agree, got %lld x %d and %lld x %d", (long long)N, V,
                    (long long)n_samples_b, n_features_b);
    CK(check_n_draws(B));
    if (conv_test_freq >= 1 && max_iterations >= 0 && max_iterations % conv_test_freq != 0)
        return fail("max_iterations must be a multiple of conv_test_freq, got %d and %d", max_iterations, conv_test_freq);
    // the host ends of the asynchronous copies live until d's destructor has waited for the stream: d is declared after them
    RefitInputs in, in_b;
    CK(refit_prepare(device, counts_a, N, V, signatures, K, 0, 0, nullptr, min_iterations, max_iterations, conv_test_freq, tol, true, in,
                     AssignSets{candidates, nullptr, 0}));
    CK(refit_prepare(device, counts_b, N, V, signatures, K, 0, 0, nullptr, min_iterations, max_iterations, conv_test_freq, tol, true, in_b));
    CK(presence_check_test(test, S, K));
    CK(refit_check_counts(counts_a, N, V, in.icounts));  // integer counts, row totals below 2^32
    CK(refit_check_counts(counts_b, N, V, in_b.icounts));
    const int cus = in.cus;

    // the tested problems: s a candidate and not the only one (the presence test's list), and a positive total on either side
    std::vector<int> pair_n, pair_s;
    std::vector<size_t> slot;
    presence_list_pairs(in, N, K, test, S, candidates != nullptr, tested, pair_n, pair_s, slot);
    {
        size_t kept = 0;
        for (size_t j = 0; j < pair_n.size(); ++j) {
            const size_t n = (size_t)pair_n[j];
            uint64_t total_a = 0, total_b = 0;
            for (int v = 0; v < V; ++v) total_a += in.icounts[n * V + v], total_b += in_b.icounts[n * V + v];
            if (total_a > 0 && total_b > 0)
                pair_n[kept] = pair_n[j], pair_s[kept] = pair_s[j], slot[kept] = slot[j], ++kept;
            else
                tested[slot[j]] = 0;
        }
        pair_n.resize(kept), pair_s.resize(kept), slot.resize(kept);
    }
    const size_t NP = pair_n.size();
    if (NP > 0x3fffffff) return fail("%zu tested problems: at most 2^30 - 1", NP);  // (the draw's grid: two workgroups per problem)
    const double nan = std::nan("");
    const size_t NS = (size_t)N * S, NK = (size_t)N * K, NB = NS * B;
    std::fill(statistic, statistic + NS, nan);
    std::fill(null_mean, null_mean + NS, nan);
    std::fill(n_exceed, n_exceed + NS, 0);
    std::fill(exposures_a, exposures_a + NK, nan);
    std::fill(exposures_b, exposures_b + NK, nan);
    std::fill(tied_exposures_a, tied_exposures_a + NS * K, nan);
    std::fill(tied_exposures_b, tied_exposures_b + NS * K, nan);
    std::fill(errors, errors + 4 * NS, nan);
    std::fill(n_iterations, n_iterations + 3 * NS, 0);
    std::fill(converged, converged + 3 * NS, 0);
    std::fill(null_statistics, null_statistics + NB, nan);
    std::fill(null_n_iterations, null_n_iterations + 3 * NB, 0);
    if (draws) std::fill(draws, draws + 2 * NB * V, 0.0);
    if (timings) timings[0] = timings[1] = timings[2] = timings[3] = 0.0;
    if (NP == 0) return 0;

    // draws per chunk: the [chunk][problems][2][V] buffer stays within chunk_bytes (at least one draw)
    const size_t PV2 = NP * 2 * V, PK = NP * K, PB = NP * B;
    const int chunk = (int)chunk_rows(chunk_bytes, sizeof(double) * PV2, B);
    std::vector<double> h_stat(NP), h_f(4 * NP), h_Ha(PK), h_Hb(PK), h_Ha0(PK), h_Hb0(PK), h_mean(NP), h_stat_b(PB), h_draws(draws ? PB * 2 * V : 0);
    std::vector<int> h_nit(3 * NP), h_conv(3 * NP), h_exceed(NP), h_nit_b(3 * PB);

    DevBufs d;
    CK(d.own_stream());
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dXa = upload(d, in.x);
    double* dXb = upload(d, in_b.x);
    int* dpn = upload(d, pair_n);
    int* dps = upload(d, pair_s);
    uint32_t* dcand = candidates ? upload(d, in.cand) : nullptr;
    double* dstat = d.get<double>(NP);
    double* df = d.get<double>(4 * NP);
    int* dnit = d.get<int>(3 * NP);
    int* dconv = d.get<int>(3 * NP);
    double* dHa = d.get<double>(PK);
    double* dHb = d.get<double>(PK);
    double* dHa0 = d.get<double>(PK);
    double* dHb0 = d.get<double>(PK);
    unsigned* dnext = d.get<unsigned>(1);
    double* dXd = d.get<double>((size_t)chunk * PV2);
    double* dstat_b = d.get<double>(PB);
    int* dnit_b = d.get<int>(3 * PB);
    int* dexceed = d.get<int>(NP);
    double* dmean = d.get<double>(NP);
    if (!dW || !dXa || !dXb || !dpn || !dps || (candidates && !dcand) || !dstat || !df || !dnit || !dconv || !dHa || !dHb || !dHa0 || !dHb0 || !dnext ||
        !dXd || !dstat_b || !dnit_b || !dexceed || !dmean)
        return fail("hipMalloc or upload failed (%d draws of %zu problems x 2 x %d, %d signatures)", B, NP, V, K);

    Spans sp;  // draw, solve, reduce
    sp.start(d, timings != nullptr);
    const SigChangeArgs a{dXa, dXb, dW, dpn, dps, dcand, dstat, dnit, df, dconv, dHa, dHb, dHa0, dHb0, dnext, (int64_t)NP, (int64_t)NP, (int64_t)V, V, K, 1,
                          min_iterations, max_iterations, conv_test_freq, tol};
    CK(sp.timed(1, [&] { return launch_sigchange(a, cus, d.stream); }));
    int n_chunks = 0;
    for (int first = 0; first < B; first += chunk, ++n_chunks) {
        const int count = std::min(chunk, B - first);
        // from the device-resident exposures of the observed tied fits; a side's trial count is read off its clipped counts
        CK(sp.timed(0, [&]() -> int {
            sigchange_launch_draw(dHa0, dHb0, dW, dXa, dXb, dpn, dps, dXd, (int64_t)NP, V, K, seed, SALNMF_EPSILON, first, count, d.stream);
            HIPCK(hipGetLastError());
            return 0;
        }));
        if (draws) CK(download(d, h_draws.data() + (size_t)first * PV2, dXd, (size_t)count * PV2));
        SigChangeArgs c = a;
        c.Xa = dXd, c.Xb = dXd + V, c.stride = 2 * (int64_t)V, c.by_sample = 0;
        c.P = (int64_t)count * (int64_t)NP;
        c.stat = dstat_b + (size_t)first * NP;
        c.nit = dnit_b + 3 * (size_t)first * NP;
        c.f = nullptr, c.conv = nullptr, c.Ha = nullptr, c.Hb = nullptr, c.Ha0 = nullptr, c.Hb0 = nullptr;
        CK(sp.timed(1, [&] { return launch_sigchange(c, cus, d.stream); }));
    }
    // gof_reduce_kernel over the problems: n_exceed counts t_b >= t (false for a NaN on either side), null_mean sums from 0.0 in ascending b
    const GofReduceArgs red{dstat, dstat_b, dexceed, dmean, (int64_t)NP, B};
    CK(sp.timed(2, [&]() -> int {
        gof_launch_reduce(red, d.stream);
        HIPCK(hipGetLastError());
        return 0;
    }));
    CK(download(d, h_stat, dstat));
    CK(download(d, h_f, df));
    CK(download(d, h_nit, dnit));
    CK(download(d, h_conv, dconv));
    CK(download(d, h_Ha, dHa));
    CK(download(d, h_Hb, dHb));
    CK(download(d, h_Ha0, dHa0));
    CK(download(d, h_Hb0, dHb0));
    CK(download(d, h_exceed, dexceed));
    CK(download(d, h_mean, dmean));
    CK(download(d, h_stat_b, dstat_b));
    CK(download(d, h_nit_b, dnit_b));
    HIPCK(hipStreamSynchronize(d.stream));

    // the compact problem list back into the (N, S, ...) results; a sample's free fits are those of its first tested problem (every
    // tested problem of a pair solves the same two rows on C and holds the same bits)
    for (size_t j = 0; j < NP; ++j) {
        const size_t o = slot[j], n = (size_t)pair_n[j];
        if (j == 0 || pair_n[j - 1] != pair_n[j]) {
            std::copy(h_Ha.begin() + j * K, h_Ha.begin() + (j + 1) * K, exposures_a + n * K);
            std::copy(h_Hb.begin() + j * K, h_Hb.begin() + (j + 1) * K, exposures_b + n * K);
        }
        statistic[o] = h_stat[j];
        n_exceed[o] = h_exceed[j];
        null_mean[o] = h_mean[j];
        std::copy(h_Ha0.begin() + j * K, h_Ha0.begin() + (j + 1) * K, tied_exposures_a + o * K);
        std::copy(h_Hb0.begin() + j * K, h_Hb0.begin() + (j + 1) * K, tied_exposures_b + o * K);
        for (int i = 0; i < 4; ++i) errors[4 * o + i] = h_f[4 * j + i];
        for (int i = 0; i < 3; ++i) n_iterations[3 * o + i] = h_nit[3 * j + i], converged[3 * o + i] = h_conv[3 * j + i];
        for (size_t b = 0; b < (size_t)B; ++b) {
            null_statistics[b * NS + o] = h_stat_b[b * NP + j];
            for (int i = 0; i < 3; ++i) null_n_iterations[3 * (b * NS + o) + i] = h_nit_b[3 * (b * NP + j) + i];
            if (draws)  // plain counts: the clipped zeros restored to 0
                for (int i = 0; i < 2 * V; ++i) {
                    const double c = h_draws[(b * NP + j) * 2 * V + i];
                    draws[(b * NS + o) * 2 * V + i] = c < 1.0 ? 0.0 : c;
                }
        }
    }
    CK(sp.totals(3, timings));
    if (timings) timings[3] = (double)n_chunks;
    return 0;
}
