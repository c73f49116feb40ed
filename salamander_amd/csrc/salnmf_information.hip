// Host side of the exposure covariance (include/salnmf.h: salnmf_exposure_covariance) and the instantiations of its kernel
// (salnmf_information.h: information_kernel), DESIGN.md section 20.  A translation unit of its own: the tile-solve kernels of
// salnmf_refit.hip fill the register file, and nothing added here can move their allocation.  The driver is written with the
// refit family's host kit (salnmf_host_kit.h: Spans, chunk_rows, upload / download).
#define SALNMF_TEMPLATES_ONLY 1
#define SALNMF_INFORMATION_KERNELS 1
#include "../../include/salnmf.h"
#include "salnmf_kernels.h"
#include "salnmf_device.h"
#include "salnmf_host_kit.h"
#include "salnmf_information.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

using namespace salnmf;

namespace {

// One workgroup per CU, at most one per sample; the ticket reset; the instantiation for (K + 15) / 16 signature tiles
int launch_information(const InfoArgs& a, int cus, hipStream_t stream) {
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)cus, a.count));
    HIPCK(hipMemsetAsync(a.next, 0, sizeof(unsigned), stream));
    switch ((a.K + 15) / 16) {
        case 1: hipLaunchKernelGGL(information_kernel<1>, grid, dim3(BLOCK), 0, stream, a); break;
        case 2: hipLaunchKernelGGL(information_kernel<2>, grid, dim3(BLOCK), 0, stream, a); break;
        case 3: hipLaunchKernelGGL(information_kernel<3>, grid, dim3(BLOCK), 0, stream, a); break;
        case 4: hipLaunchKernelGGL(information_kernel<4>, grid, dim3(BLOCK), 0, stream, a); break;
        case 5: hipLaunchKernelGGL(information_kernel<5>, grid, dim3(BLOCK), 0, stream, a); break;
        case 6: hipLaunchKernelGGL(information_kernel<6>, grid, dim3(BLOCK), 0, stream, a); break;
        default: return fail("no information kernel for %d signatures", a.K);
    }
    HIPCK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int salnmf_exposure_covariance(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures, int n_signatures,
                                          const double* exposures, const unsigned char* active, int information, double min_pivot, int64_t chunk_bytes,
                                          double* standard_errors, double* inflation, double* information_diag, double* max_abs_correlation,
                                          int* most_confounded, double* min_pivot_value, int* singular, int* n_active, double* correlation,
                                          double* timings) {
    const int64_t N = n_samples;
    const int V = n_features, K = n_signatures;
    if (!counts || !signatures || !exposures || !active || !standard_errors || !inflation || !information_diag || !max_abs_correlation ||
        !most_confounded || !min_pivot_value || !singular || !n_active)
        return fail("null argument");
    if (N < 1 || N > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)N);
    if (V < 1 || V > VMAX) return fail("n_features must be in [1, %d], got %d", VMAX, V);
    if (K < 1 || K > INFO_KMAX) return fail("n_signatures must be in [1, %d], got %d", INFO_KMAX, K);
    if (information != 0 && information != 1) return fail("information must be 0 (observed) or 1 (expected), got %d", information);
    if (!std::isfinite(min_pivot) || !(min_pivot > 0.0 && min_pivot < 1.0)) return fail("min_pivot must lie in (0, 1), got %g", min_pivot);
    for (int k = 0; k < K; ++k) {
        double sum = 0.0;
        for (int v = 0; v < V; ++v) {
            const double w = signatures[(size_t)k * V + v];
            if (!std::isfinite(w) || w < 0.0) return fail("signature %d, feature %d: entries must be finite and not negative, got %g", k, v, w);
            sum += w;
        }
        if (!(sum > 0.0) || !std::isfinite(sum)) return fail("signature %d needs a positive finite sum", k);
    }
    std::vector<double> x((size_t)N * V);
    for (size_t i = 0; i < x.size(); ++i) {
        if (!std::isfinite(counts[i]) || counts[i] < 0.0)
            return fail("counts must be finite and not negative: row %lld, column %d holds %g", (long long)(i / V), (int)(i % V), counts[i]);
        x[i] = counts[i] < SALNMF_EPSILON ? SALNMF_EPSILON : counts[i];
    }
    const size_t NK = (size_t)N * K, KK = (size_t)K * K;
    for (size_t i = 0; i < NK; ++i)
        if (!std::isfinite(exposures[i]) || exposures[i] < 0.0)
            return fail("exposures must be finite and not negative: row %lld, signature %d holds %g", (long long)(i / K), (int)(i % K), exposures[i]);
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    const int cus = prop.multiProcessorCount;

    // samples per launch: with the correlations asked for, the [chunk][K][K] buffer stays within chunk_bytes (at least one sample)
    const int64_t chunk = correlation ? chunk_rows(chunk_bytes, sizeof(double) * KK, N) : N;

    DevBufs d;
    CK(d.own_stream());
    double* dW = upload(d, signatures, (size_t)K * V);
    double* dX = upload(d, x);
    double* dH = upload(d, exposures, NK);
    uint8_t* dact = upload(d, (const uint8_t*)active, NK);
    double* dse = d.get<double>(NK);
    double* dinfl = d.get<double>(NK);
    double* dinfo = d.get<double>(NK);
    double* dmaxc = d.get<double>(NK);
    int* dconf = d.get<int>(NK);
    double* dminp = d.get<double>((size_t)N);
    int* dsing = d.get<int>((size_t)N);
    int* dnact = d.get<int>((size_t)N);
    unsigned* dnext = d.get<unsigned>(1);
    double* dcorr = correlation ? d.get<double>((size_t)chunk * KK) : nullptr;
    if (!dW || !dX || !dH || !dact || !dse || !dinfl || !dinfo || !dmaxc || !dconf || !dminp || !dsing || !dnact || !dnext || (correlation && !dcorr))
        return fail("hipMalloc or upload failed (covariance of %lld samples, %d signatures)", (long long)N, K);

    InfoArgs a{dX, dW, dH, dact, dse, dinfl, dinfo, dmaxc, dconf, dminp, dsing, dnact, dcorr, dnext, 0, 0, V, K, information, min_pivot};
    Spans sp;  // the kernel
    sp.start(d, timings != nullptr);
    int n_chunks = 0;
    for (int64_t first = 0; first < N; first += chunk, ++n_chunks) {
        a.first = first, a.count = std::min(chunk, N - first);
        CK(sp.timed(0, [&] { return launch_information(a, cus, d.stream); }));
        if (correlation) CK(download(d, correlation + (size_t)first * KK, dcorr, (size_t)a.count * KK));
    }
    CK(download(d, standard_errors, dse, NK));
    CK(download(d, inflation, dinfl, NK));
    CK(download(d, information_diag, dinfo, NK));
    CK(download(d, max_abs_correlation, dmaxc, NK));
    CK(download(d, most_confounded, dconf, NK));
    CK(download(d, min_pivot_value, dminp, (size_t)N));
    CK(download(d, singular, dsing, (size_t)N));
    CK(download(d, n_active, dnact, (size_t)N));
    HIPCK(hipStreamSynchronize(d.stream));
    CK(sp.totals(1, timings));
    if (timings) timings[1] = (double)n_chunks;
    return 0;
}
