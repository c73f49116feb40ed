// Host side of the signature-presence test under the negative-binomial likelihood (include/salnmf.h:
// salnmf_nb_signature_presence) and the instantiations of its kernel (salnmf_nb_presence.h: nb_presence_kernel), DESIGN.md section
// 26.  A translation unit of its own, as salnmf_nb.hip and salnmf_nb_assign.hip are: the tile-solve kernels of the other units fill
// the register file, and nothing added here can move their allocation.  The entry point is salnmf_signature_presence's driver
// (salnmf_refit_drivers.h: the pair run) with NbPresenceArgs and this unit's model object: the dispersions checked where
// salnmf_nb_refit_exposures checks them, alpha and the gamma draw's constants uploaded, nb_presence_kernel for the solves,
// nb_presence_draw_kernel (salnmf_batch.hip) for the draws, the bound on the null fits' means between the observed launch and the
// first draw, and the count of rows no draw could be made for.  gof_reduce_kernel (salnmf_batch.hip) reduces.
#define SALNMF_TEMPLATES_ONLY 1
#define SALNMF_REFIT_KERNELS 1
#define SALNMF_NB_KERNELS 1
#define SALNMF_NB_PIECES_ONLY 1
#include "../../include/salnmf.h"
#include "salnmf_kernels.h"
#include "salnmf_device.h"
#include "salnmf_refit_drivers.h"
#include "salnmf_nb_presence.h"

#include <algorithm>
#include <cstdint>
#include <vector>

using namespace salnmf;

namespace {

struct NbPresence {
    const double* dispersion;  // [N]
    int64_t N;
    std::vector<double> gd, gc;  // (host ends of asynchronous copies: this object is declared before the run that owns the stream)
    unsigned zero = 0, failed = 0;
    double *dalpha = nullptr, *dgd = nullptr, *dgc = nullptr;
    unsigned* dfailed = nullptr;

    int own_checks() const { return nb_check_dispersion(dispersion, N); }
    bool inputs(DevBufs& d, NbPresenceArgs& a) {
        nb_gamma_constants(dispersion, N, gd, gc);
        dalpha = upload(d, dispersion, (size_t)N);  // (not tiled: a problem reads its sample's)
        dgd = upload(d, gd);
        dgc = upload(d, gc);
        dfailed = upload(d, &zero, 1);
        a.alpha = dalpha;
        return dalpha && dgd && dgc && dfailed;
    }
    int launch(const NbPresenceArgs& a, int cus, hipStream_t stream) const {
        return launch_tiles("negative-binomial presence", a.P, a.K, a.next_tile, cus, stream,
                            [&](auto kt, dim3 grid) { hipLaunchKernelGGL(nb_presence_kernel<decltype(kt)::value>, grid, dim3(BLOCK), 0, stream, a); });
    }
    // The draw's bound (salnmf_draw_nb_counts'): a null fit whose model row sums to more than 2^24 is refused before any draw.
    // The observed launch is waited for.
    int after_observed(const PairIO& io, PairRunOf<NbPresenceArgs>& r) const {
        DevBufs& d = *r.d;
        CK(download(d, r.h_H0, r.dH0));
        HIPCK(hipStreamSynchronize(d.stream));
        r.h0_on_host = true;  // (the driver does not copy it again)
        for (size_t j = 0; j < r.NP; ++j) {
            const double mean = nb_model_row_sum(r.h_H0.data() + j * io.K, io.signatures, io.K, io.V);
            if (!(mean <= NB_MAX_MEAN))
                return fail("the null fits' row sums must not exceed 2^24: sample %d without signature %d sums to %g", r.pair_n[j], r.pair_s[j], mean);
        }
        return 0;
    }
    void draw(PairRunOf<NbPresenceArgs>& r, uint64_t seed, int first, int count) const {
        nb_presence_launch_draw(r.dH0, r.dW, dalpha, dgd, dgc, r.dpn, r.dps, r.dXb, dfailed, (int64_t)r.NP, r.a.V, r.a.K, seed, SALNMF_EPSILON, first,
                                count, r.d->stream);
    }
    int before_wait(DevBufs& d) { return download(d, &failed, dfailed, 1); }
};

}  // namespace

extern "C" int salnmf_nb_signature_presence(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                                            int n_signatures, const double* dispersion, const int* test, int n_test, const uint8_t* candidates, int n_draws,
                                            uint64_t seed, int min_iterations, int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes,
                                            uint8_t* tested, double* statistic, int* n_exceed, double* null_mean, double* exposures, double* errors,
                                            double* null_exposures, double* null_errors, int* n_iterations, int* converged, double* null_statistics,
                                            int* null_n_iterations, double* draws, double* timings, int* n_failed) {
    if (!dispersion || !n_failed) return fail("null argument");
    const PairIO io{device, counts, n_samples, n_features, signatures, n_signatures, test, n_test, candidates, min_iterations, max_iterations,
                    conv_test_freq, tol, tested, exposures, errors, timings, n_draws, seed, chunk_bytes, statistic, n_exceed, null_mean, null_exposures,
                    null_errors, n_iterations, converged, null_statistics, null_n_iterations, draws};
    NbPresence m{dispersion, n_samples};
    PairRunOf<NbPresenceArgs> r;
    *n_failed = 0;
    CK(presence_enqueue(io, 0, r, m));
    if (r.NP == 0) return 0;
    CK(presence_finish(io, r));
    *n_failed = (int)std::min<unsigned>(m.failed, 0x7fffffffu);
    return 0;
}
