// KLNMFSweep on the device: the batch handle of include/salnmf.h (salnmf_batch_*), the batched objective / per-sample
// divergence passes, and the host side of the batched step (its kernel: salnmf_small.hip, small_kl_batch_kernel).
// Layout and the bit-for-bit argument: salnmf_batch.h, DESIGN.md section 12.  Also the host side of the two count draws --
// the bootstrap resampler (salnmf_resample.h) and count splitting (salnmf_split.h), which share one kernel body
// (count_draw_row) and here one driver per job (draw_into_slots, draw_stand_alone, profile_draw: a draw is its argument check
// and the callable that launches its kernel) -- and of the signature-stability kernel (salnmf_stability.h).
#define SALNMF_TEMPLATES_ONLY 1
#include "../../include/salnmf.h"
#include "salnmf_batch.h"
#include "salnmf_device.h"
#include "salnmf_refit.h"
#include "salnmf_resample.h"
#include "salnmf_split.h"
#define SALNMF_GOF_KERNELS 1
#include "salnmf_gof.h"
#define SALNMF_NBDRAW_KERNELS 1
#include "salnmf_nbdraw.h"
#include "salnmf_presence.h"
#include "salnmf_nb_presence.h"
#include "salnmf_change.h"
#include "salnmf_sigchange.h"
#include "salnmf_power.h"
#include "salnmf_stability.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace salnmf;

namespace salnmf {
namespace {

// one launch of the batched forward pass: blockIdx.y = entry of `active`, blockIdx.x = the workgroup of that member's
// pass (gridDim.x = the engine's forward_grid for this shape)
struct BatchFwdArgs {
    const BatchMember* __restrict__ members;
    const int* __restrict__ active;
    double* out;                        // mode 0: [n_members][gridDim.x] workgroup partials; mode 1: [n_members][Np]
    unsigned* counter;                  // mode 0: [n_members] arrival counters, zero between launches
    double* sum_out;                    // mode 0: row `slot` of the objective array, [n_members] (pinned host memory)
    int64_t N, ntiles;
    int V;
    // held-out scoring (salnmf_batch_heldout_kl), null for every other launch: entry blockIdx.y of `xover` is the
    // [Np][96] matrix the member is evaluated against instead of its own dataset, and `hscale` ([16], mode 1 only) the
    // exposure scale H is read with, as clip(H * hscale)
    const double* const* __restrict__ xover;
    const double* __restrict__ hscale;
    // mode 0: the weight table of the batched step (salnmf_batch.h: SmallBatchArgs::weights); null for mode 1
    const double* const* __restrict__ weights;
};

// forward_body<KS, MODE> (salnmf_forward_kernel.h) for one member with the parameters an engine of <= 16 signatures and
// <= 96 features passes for salnmf_objective_async (mode 0, the in-launch sum) and salnmf_samplewise_kl (mode 1):
// the member's own dataset, no pending exposure scale, one feature block, one signature chunk; mode 0 with the member's
// weights (salnmf_batch_set_weights: the weighted KL and the l-half penalty of an engine's objective), mode 1 always
// unweighted, as salnmf_samplewise_kl.  Members of
// 1-4, 5-8 and 9-16 signatures share the launch (KS = 1, 2, 4; the branch is uniform per workgroup, LDS is sized for the
// widest).
template <int MODE>
__global__ void __launch_bounds__(BLOCK, 2) batch_forward_kernel(BatchFwdArgs a) {
    static_assert(fwd_lds_doubles<4>() * 8 <= 80 * 1024, "two workgroups per CU, as forward_kernel at KS <= 4");
    __shared__ __attribute__((aligned(16))) double lds[fwd_lds_doubles<4>()];
    const int m = a.active[blockIdx.y];
    const BatchMember& b = a.members[m];
    FwdParams p{};
    p.X = a.xover ? a.xover[blockIdx.y] : b.X;
    if (MODE == 1) p.hscale = a.hscale;
    p.H = b.H;
    p.W = b.W;
    p.xlx = b.xlx;  // [Np][16] (mode 0)
    p.out = a.out + (MODE == 0 ? (size_t)m * gridDim.x : (size_t)m * 16 * a.ntiles);
    p.N = a.N;
    p.V = p.ldw = a.V;
    p.K = b.K;
    p.ntiles = a.ntiles;
    if (MODE == 0) {
        p.wkl = a.weights[2 * m];
        p.wlh = a.weights[2 * m + 1];
        p.sum_out = a.sum_out + m;
        p.sum_counter = a.counter + m;
    }
    if (b.K <= 4)
        forward_body<1, MODE, false>(p, lds);
    else if (b.K <= 8)
        forward_body<2, MODE, false>(p, lds);
    else
        forward_body<4, MODE, false>(p, lds);
}

}  // namespace
}  // namespace salnmf

struct salnmf_batch {
    int device = 0, V = 0, M = 0;
    int64_t N = 0, Np = 0, ntiles = 0;
    int fgrid = 0;  // workgroups of an engine's forward pass at this shape (forward_grid): the objective's summation order
    std::vector<int> K;
    std::vector<BatchMember> members;
    hipStream_t stream = nullptr;
    double *X = nullptr, *xlx = nullptr, *state = nullptr, *part = nullptr, *klout = nullptr;
    unsigned* counter = nullptr;
    BatchMember* dmembers = nullptr;
    int *dstep = nullptr, *dobj = nullptr;  // [2 M]: active list | n_given of the steps; [M] active list of the objectives
    std::vector<int> step_list, obj_list;   // what dstep / dobj hold
    double* pin = nullptr;                  // [SALNMF_BATCH_SLOTS][M] pinned: the queued objectives
    std::vector<hipEvent_t> ev;             // per slot: completion of the launch that wrote it
    std::vector<char> queued;
    bool x_ok = false;
    // bootstrap resamples of X (salnmf_batch_resample): R slots in X's layout, the counts they were drawn from, and the
    // dataset each member reads (-1: the uploaded X); the device's member table is rewritten before the next launch
    std::vector<double> hostX;  // [N][V] as uploaded, unclipped
    double *Xr = nullptr, *xlxr = nullptr;
    int R = 0;  // slots: the resamples, or 2 F after a split
    int F = 0;  // count splitting (salnmf_batch_split): train split f is dataset f, test split f dataset F + f
    std::vector<int> dataset;
    bool members_dirty = false;
    // per-member weights (salnmf_batch_set_weights): device arrays of Np doubles, pad rows 1 / 0, null without weights;
    // entries 2 m, 2 m + 1 = member m's w_kl, w_lhalf.  dweights is the device's copy, rewritten with the member table
    std::vector<double*> weights;
    const double** dweights = nullptr;
};

// the device's member table follows the host's once the launches that read the old one are done
static int flush_members(salnmf_batch* b) {
    if (!b->members_dirty) return 0;
    HIPCK(hipStreamSynchronize(b->stream));
    HIPCK(hipMemcpy(b->dmembers, b->members.data(), b->members.size() * sizeof(BatchMember), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(b->dweights, b->weights.data(), b->weights.size() * sizeof(double*), hipMemcpyHostToDevice));
    b->members_dirty = false;
    return 0;
}

// dataset d of a batch: slot d of the resamples or split halves, -1 the uploaded X
static const double* dataset_ptr(const salnmf_batch* b, int d) { return d < 0 ? b->X : b->Xr + (size_t)d * b->Np * VMAX; }

static int check_dataset(const salnmf_batch* b, int d) {
    if (d < -1 || d >= b->R) return fail("dataset %d out of range (%d resamples or split halves; -1 is the uploaded X)", d, b->R);
    return 0;
}

static void point_member(salnmf_batch* b, int m, int dataset) {
    BatchMember& mb = b->members[(size_t)m];
    mb.X = dataset_ptr(b, dataset);
    mb.xlx = dataset < 0 ? b->xlx : b->xlxr + (size_t)dataset * b->Np * 16;
    b->dataset[(size_t)m] = dataset;
    b->members_dirty = true;
}

// the resamples go with the X they were drawn from: every member is back on the uploaded X
static void drop_resamples(salnmf_batch* b) {
    for (int m = 0; m < b->M; ++m)
        if (b->dataset[(size_t)m] >= 0) point_member(b, m, -1);
    if (b->Xr) (void)hipFree(b->Xr);
    if (b->xlxr) (void)hipFree(b->xlxr);
    b->Xr = b->xlxr = nullptr;
    b->R = b->F = 0;
}

// Counts a resample can be drawn from: integer values, none negative, row totals below 2^32.  The counts as uint32.
static int check_counts(const double* X, int64_t N, int V, std::vector<uint32_t>& counts) {
    counts.resize((size_t)N * V);
    for (int64_t n = 0; n < N; ++n) {
        uint64_t total = 0;
        for (int v = 0; v < V; ++v) {
            const double x = X[(size_t)n * V + v];
            if (!(x >= 0.0) || x >= 4294967296.0 || x != (double)(uint64_t)x)
                return fail("resampling needs non-negative integer counts below 2^32: row %lld, column %d holds %g", (long long)n, v, x);
            total += (uint64_t)x;
            counts[(size_t)n * V + v] = (uint32_t)x;
        }
        if (total >> 32) return fail("resampling needs row totals below 2^32: row %lld sums to %llu", (long long)n, (unsigned long long)total);
    }
    return 0;
}

static int check_resample_args(int n_resamples) {
    // (one workgroup per (row, resample): the resample is the grid's y)
    if (n_resamples < 1 || n_resamples > 65535) return fail("n_resamples must be in [1, 65535], got %d", n_resamples);
    return 0;
}

static int check_split_args(int n_splits, uint64_t thr) {
    // (one workgroup per (row, split), two slots per split: the split is the grid's y)
    if (n_splits < 1 || n_splits > 32767) return fail("n_splits must be in [1, 32767], got %d", n_splits);
    if (thr == 0) return fail("the train threshold must be in [1, 2^64 - 1]: train_fraction * 2^64 rounds to 0");
    return 0;
}

static int check_member(const salnmf_batch* b, int m) {
    if (!b) return fail("null batch");
    if (m < 0 || m >= b->M) return fail("member %d out of range (%d members)", m, b->M);
    return 0;
}

// a list of n member indices, each in range and none twice
static int check_list(const salnmf_batch* b, int n, const int* members) {
    if (n < 0 || n > b->M) return fail("%d members listed, the batch has %d", n, b->M);
    if (n > 0 && !members) return fail("null member list");
    std::vector<char> seen((size_t)b->M, 0);
    for (int i = 0; i < n; ++i) {
        CK(check_member(b, members[i]));
        if (seen[(size_t)members[i]]++) return fail("member %d listed twice", members[i]);
    }
    return 0;
}

// a device list is rewritten only when it changes -- after the host has read objectives and dropped converged members --
// and only once the launches that read its old content are done
static int set_list(salnmf_batch* b, int* dev, std::vector<int>& cache, const std::vector<int>& want) {
    if (cache == want) return 0;
    HIPCK(hipStreamSynchronize(b->stream));
    HIPCK(hipMemcpy(dev, want.data(), want.size() * sizeof(int), hipMemcpyHostToDevice));
    cache = want;
    return 0;
}

// ---- the count draws (salnmf_resample.h, salnmf_split.h): one driver per job, the draw being the callable that launches it

// The uploaded counts drawn into n_slots fresh datasets.  `launch(dcounts)` queues the kernel that fills b->Xr straight in X's
// layout: pad rows and columns 0, the N x V block clipped as upload_X(clip = 1) clips.  A failure leaves the batch without slots.
template <typename Launch>
static int draw_into_slots(salnmf_batch* b, int n_slots, Launch launch) {
    // (host buffer of the asynchronous copy: declared before d, so it outlives its wait for the stream)
    std::vector<uint32_t> counts;
    CK(check_counts(b->hostX.data(), b->N, b->V, counts));
    HIPCK(hipSetDevice(b->device));
    HIPCK(hipStreamSynchronize(b->stream));
    drop_resamples(b);
    DevBufs d(b->stream);
    const size_t xsz = (size_t)b->Np * VMAX, csz = (size_t)b->Np * 16;
    auto draw = [&]() -> int {
        uint32_t* dcounts = d.get<uint32_t>(counts.size());
        if (!dcounts || hipMalloc(&b->Xr, (size_t)n_slots * xsz * sizeof(double)) != hipSuccess ||
            hipMalloc(&b->xlxr, (size_t)n_slots * csz * sizeof(double)) != hipSuccess)
            return fail("hipMalloc failed (%d datasets)", n_slots);
        HIPCK(hipMemcpyAsync(dcounts, counts.data(), counts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
        launch(dcounts);
        HIPCK(hipGetLastError());
        for (int s = 0; s < n_slots; ++s) {
            launch_xlogx_lane(b->Xr + (size_t)s * xsz, b->Np, b->V, b->xlxr + (size_t)s * csz, b->stream);
            HIPCK(hipGetLastError());
        }
        HIPCK(hipStreamSynchronize(b->stream));
        return 0;
    };
    const int rc = draw();
    if (rc) drop_resamples(b);
    return rc;
}

// The draws of a stand-alone count matrix, compact and unclipped: `launch(dcounts, dout)` fills dout, and its first n_out
// doubles go to out0, the next n_out to out1 where there is a second output.
template <typename Launch>
static int draw_stand_alone(int device, const double* X, int64_t n_samples, int n_features, int n_draws, double* out0, double* out1, Launch launch) {
    if (n_samples < 1 || n_samples > 0x7fffffff) return fail("n_samples must be in [1, 2^31), got %lld", (long long)n_samples);
    if (n_features < 1 || n_features > RESAMPLE_VMAX) return fail("n_features must be in [1, %d], got %d", RESAMPLE_VMAX, n_features);
    std::vector<uint32_t> counts;
    CK(check_counts(X, n_samples, n_features, counts));
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    DevBufs d;
    const size_t n_out = (size_t)n_draws * counts.size();
    uint32_t* dcounts = d.get<uint32_t>(counts.size());
    double* dout = d.get<double>((out1 ? 2 : 1) * n_out);
    if (!dcounts || !dout) return fail("hipMalloc failed (%d draws of %lld x %d)", n_draws, (long long)n_samples, n_features);
    HIPCK(hipMemcpy(dcounts, counts.data(), counts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    launch(dcounts, dout);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(out0, dout, n_out * sizeof(double), hipMemcpyDeviceToHost));
    if (out1) HIPCK(hipMemcpy(out1, dout + n_out, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// Development aid: the average milliseconds of one launch of a draw's kernel, by device events.  `draw()` is the batch's own
// entry point (it validates, allocates the slots and warms the kernel up), `launch(dcounts)` what it queues.
template <typename Draw, typename Launch>
static int profile_draw(salnmf_batch* b, int n_calls, double* avg_ms, Draw draw, Launch launch) {
    if (!b || !avg_ms) return fail("null argument");
    if (!b->x_ok) return fail("upload X first");
    if (n_calls < 1) return fail("n_calls must be positive");
    CK(draw());
    std::vector<uint32_t> counts;
    CK(check_counts(b->hostX.data(), b->N, b->V, counts));
    DevBufs d(b->stream);
    uint32_t* dcounts = d.get<uint32_t>(counts.size());
    if (!dcounts) return fail("hipMalloc failed");
    HIPCK(hipMemcpy(dcounts, counts.data(), counts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    const hipEvent_t e0 = d.mark();
    for (int i = 0; i < n_calls; ++i) launch(dcounts);  // (the same bits every time)
    const hipEvent_t e1 = d.mark();
    if (!e0 || !e1) return fail("event record failed");
    HIPCK(hipGetLastError());
    HIPCK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = (double)ms / n_calls;
    return 0;
}

// what the batch queues for its draws: resample r into slot r; train split f into slot f, test split f into slot F + f
static auto batch_resample_launch(salnmf_batch* b, int n_resamples, uint64_t seed) {
    return [=](const uint32_t* dcounts) {
        launch_resample(ResampleArgs{dcounts, b->Xr, b->N, b->Np, b->V, VMAX, (uint32_t)seed, (uint32_t)(seed >> 32), SALNMF_EPSILON}, n_resamples, b->stream);
    };
}

static auto batch_split_launch(salnmf_batch* b, int n_splits, uint64_t thr, uint64_t seed) {
    return [=](const uint32_t* dcounts) {
        double* test = b->Xr + (size_t)n_splits * b->Np * VMAX;
        launch_split(SplitArgs{dcounts, b->Xr, test, b->N, b->Np, b->V, VMAX, (uint32_t)seed, (uint32_t)(seed >> 32), thr, SALNMF_EPSILON}, n_splits, b->stream);
    };
}

// ---- the resampler as salnmf_refit.hip uses it (salnmf_refit.h): this translation unit holds resample_counts_kernel
int salnmf::refit_check_counts(const double* X, int64_t N, int V, std::vector<uint32_t>& counts) { return check_counts(X, N, V, counts); }

void salnmf::refit_launch_resample(const uint32_t* counts, double* out, int64_t N, int V, uint64_t seed, int first, int count, hipStream_t stream) {
    // compact rows, no pad rows, entries max(count, EPSILON): the clip fit() applies to X
    launch_resample(ResampleArgs{counts, out, N, N, V, V, (uint32_t)seed, (uint32_t)(seed >> 32), SALNMF_EPSILON, (uint32_t)first}, count, stream);
}

// ---- the model draw and the exceedance count as salnmf_refit.hip uses them (salnmf_gof.h): philox4x32_10 comes from
// salnmf_resample.h, which this translation unit alone includes
void salnmf::gof_launch_model_draw(const double* H, const double* W, const uint32_t* totals, const double* X, double* out, int64_t N, int V, int K,
                                   uint64_t seed, double floor, int first, int count, hipStream_t stream) {
    for (int done = 0; done < count; done += GOF_GRID_Y) {
        const int now = std::min(GOF_GRID_Y, count - done);
        const ModelDrawArgs a{H, W, totals, X, out + (size_t)done * N * V, N, V, K, (uint32_t)seed, (uint32_t)(seed >> 32), floor, (uint32_t)(first + done)};
        hipLaunchKernelGGL(model_draw_kernel, dim3((unsigned)N, (unsigned)now), dim3(RESAMPLE_BLOCK), 0, stream, a);
    }
}

void salnmf::gof_launch_reduce(const GofReduceArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(gof_reduce_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, stream, a);
}

// the negative-binomial model draw (salnmf_nbdraw.h), as salnmf_nb.hip uses it: one workgroup per (row, draw)
void salnmf::nb_launch_draw(const double* H, const double* W, const double* alpha, const double* gd, const double* gc, double* out, unsigned* failed, int64_t N,
                            int V, int K, uint64_t seed, double floor, int first, int count, hipStream_t stream) {
    for (int done = 0; done < count; done += GOF_GRID_Y) {
        const int now = std::min(GOF_GRID_Y, count - done);
        const NbDrawArgs a{H, W, alpha, gd, gc, out + (size_t)done * N * V, failed, N, V, K, (uint32_t)seed, (uint32_t)(seed >> 32), floor, (uint32_t)(first + done)};
        hipLaunchKernelGGL(nb_draw_kernel, dim3((unsigned)N, (unsigned)now), dim3(RESAMPLE_BLOCK), 0, stream, a);
    }
}

// the presence test's draw (salnmf_presence.h): the same body, one workgroup per (pair, draw)
void salnmf::presence_launch_draw(const double* H0, const double* W, const double* X, const int* pair_n, const int* pair_s, double* out, int64_t NP, int V,
                                  int K, uint64_t seed, double floor, int first, int count, hipStream_t stream) {
    for (int done = 0; done < count; done += GOF_GRID_Y) {
        const int now = std::min(GOF_GRID_Y, count - done);
        const PresenceDrawArgs a{H0, W, X, pair_n, pair_s, out + (size_t)done * NP * V, NP, V, K, (uint32_t)seed, (uint32_t)(seed >> 32), floor,
                                 (uint32_t)(first + done)};
        hipLaunchKernelGGL(presence_draw_kernel, dim3((unsigned)NP, (unsigned)now), dim3(RESAMPLE_BLOCK), 0, stream, a);
    }
}

// the negative-binomial presence test's draw (salnmf_nb_presence.h): nb_draw_kernel's body, one workgroup per (pair, draw)
void salnmf::nb_presence_launch_draw(const double* H0, const double* W, const double* alpha, const double* gd, const double* gc, const int* pair_n,
                                     const int* pair_s, double* out, unsigned* failed, int64_t NP, int V, int K, uint64_t seed, double floor, int first,
                                     int count, hipStream_t stream) {
    for (int done = 0; done < count; done += GOF_GRID_Y) {
        const int now = std::min(GOF_GRID_Y, count - done);
        const NbPresenceDrawArgs a{H0, W, alpha, gd, gc, pair_n, pair_s, out + (size_t)done * NP * V, failed, NP, V, K, (uint32_t)seed,
                                   (uint32_t)(seed >> 32), floor, (uint32_t)(first + done)};
        hipLaunchKernelGGL(nb_presence_draw_kernel, dim3((unsigned)NP, (unsigned)now), dim3(RESAMPLE_BLOCK), 0, stream, a);
    }
}

// the change test's draw (salnmf_change.h): the same body, one workgroup per (pair, side, draw)
void salnmf::change_launch_draw(const double* H0, const double* W, const double* Xa, const double* Xb, const int* pair_n, double* out, int64_t NP, int V,
                                int K, uint64_t seed, double floor, int first, int count, hipStream_t stream) {
    for (int done = 0; done < count; done += GOF_GRID_Y) {
        const int now = std::min(GOF_GRID_Y, count - done);
        const ChangeDrawArgs a{H0, W, Xa, Xb, pair_n, out + (size_t)done * NP * 2 * V, NP, V, K, (uint32_t)seed, (uint32_t)(seed >> 32), floor,
                               (uint32_t)(first + done)};
        hipLaunchKernelGGL(change_draw_kernel, dim3((unsigned)(2 * NP), (unsigned)now), dim3(RESAMPLE_BLOCK), 0, stream, a);
    }
}

// the per-signature change test's draw (salnmf_sigchange.h): the same body, one workgroup per (problem, side, draw)
void salnmf::sigchange_launch_draw(const double* Ha0, const double* Hb0, const double* W, const double* Xa, const double* Xb, const int* pair_n,
                                   const int* pair_s, double* out, int64_t NP, int V, int K, uint64_t seed, double floor, int first, int count,
                                   hipStream_t stream) {
    for (int done = 0; done < count; done += GOF_GRID_Y) {
        const int now = std::min(GOF_GRID_Y, count - done);
        const SigChangeDrawArgs a{Ha0, Hb0, W, Xa, Xb, pair_n, pair_s, out + (size_t)done * NP * 2 * V, NP, V, K, (uint32_t)seed, (uint32_t)(seed >> 32),
                                  floor, (uint32_t)(first + done)};
        hipLaunchKernelGGL(sigchange_draw_kernel, dim3((unsigned)(2 * NP), (unsigned)now), dim3(RESAMPLE_BLOCK), 0, stream, a);
    }
}

// the power analysis of the presence test (salnmf_power.h): planting, the draw with the same body, the reduction
void salnmf::power_launch_plant(const PowerPlantArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(power_plant_kernel, dim3((unsigned)((a.NP * a.L + 255) / 256)), dim3(256), 0, stream, a);
}

void salnmf::power_launch_draw(const double* Hp, const double* W, const double* X, const int* pair_n, const int* pair_s, double* out, int64_t NP, int V,
                               int K, uint64_t seed, double floor, int n_alt_draws, int64_t first, int64_t count, hipStream_t stream) {
    for (int64_t done = 0; done < count; done += GOF_GRID_Y) {
        const int now = (int)std::min<int64_t>(GOF_GRID_Y, count - done);
        const PowerDrawArgs a{Hp, W, X, pair_n, pair_s, out + (size_t)done * NP * V, NP, V, K, (uint32_t)seed, (uint32_t)(seed >> 32), floor,
                              (uint32_t)(first + done), (uint32_t)n_alt_draws};
        hipLaunchKernelGGL(power_draw_kernel, dim3((unsigned)NP, (unsigned)now), dim3(RESAMPLE_BLOCK), 0, stream, a);
    }
}

void salnmf::power_launch_reduce(const PowerReduceArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(power_reduce_kernel, dim3((unsigned)((a.NP * a.L + 255) / 256)), dim3(256), 0, stream, a);
}

// ---- signature stability (salnmf_stability.h): the two feeders share everything after their own validation
namespace {

struct StabOut {
    int *assignments, *n_rounds, *converged;
    double *consensus, *a, *b, *silhouette, *cluster, *stability, *kernel_ms;
};

int check_stab_out(const StabOut& o) {
    if (!o.assignments || !o.n_rounds || !o.converged || !o.consensus || !o.a || !o.b || !o.silhouette || !o.cluster || !o.stability)
        return fail("null output");
    return 0;
}

// K, M of one group and the launch as a whole (one workgroup per group: the group is the grid's x)
int check_stab_group(int g, int K, int M) {
    if (K < 1 || K > STAB_K) return fail("group %d: n_signatures must be in [1, %d], got %d", g, STAB_K, K);
    if (M < 2) return fail("group %d: a group needs at least 2 members, got %d", g, M);
    return 0;
}

// One launch over all groups, then the results: per listed member [16] (assignments, a, b, silhouette), per group
// [16][96] (consensus), [16] (cluster stability), [2] (mean, minimum) and the round count / converged flag.
int run_stability(hipStream_t stream, const std::vector<StabGroup>& groups, const std::vector<const double*>& src, int ld, int V, const double* errors,
                  int max_rounds, const StabOut& o) {
    const size_t G = groups.size(), T = src.size();
    // (host buffers of the asynchronous copies: declared before d, so they outlive its wait for the stream)
    std::vector<double> err(T, 0.0), abz(3 * T * STAB_K), score(2 * G);
    std::vector<int> rounds(2 * G);
    if (errors) {
        err.assign(errors, errors + T);
        for (size_t t = 0; t < T; ++t)
            if (std::isnan(err[t])) return fail("errors must not hold NaNs (listed member %zu)", t);
    }
    DevBufs d(stream);
    StabArgs a{};
    StabGroup* dgroups = d.get<StabGroup>(G);
    const double** dsrc = d.get<const double*>(T);
    double* derr = d.get<double>(T);
    a.u = d.get<double>(T * STAB_K * VMAX);
    a.xx = d.get<double>(T * STAB_K);
    a.assign = d.get<int>(T * STAB_K);
    a.a = d.get<double>(3 * T * STAB_K);
    a.consensus = d.get<double>(G * STAB_K * VMAX);
    a.cluster = d.get<double>(G * STAB_K);
    a.score = d.get<double>(2 * G);
    a.rounds = d.get<int>(2 * G);
    if (!dgroups || !dsrc || !derr || !a.u || !a.xx || !a.assign || !a.a || !a.consensus || !a.cluster || !a.score || !a.rounds)
        return fail("hipMalloc failed (stability of %zu members in %zu groups)", T, G);
    a.b = a.a + T * STAB_K;
    a.sil = a.b + T * STAB_K;
    a.groups = dgroups;
    a.src = dsrc;
    a.err = derr;
    a.ld = ld;
    a.V = V;
    a.max_rounds = max_rounds;
    HIPCK(hipMemcpyAsync(dgroups, groups.data(), G * sizeof(StabGroup), hipMemcpyHostToDevice, stream));
    HIPCK(hipMemcpyAsync(dsrc, src.data(), T * sizeof(double*), hipMemcpyHostToDevice, stream));
    HIPCK(hipMemcpyAsync(derr, err.data(), T * sizeof(double), hipMemcpyHostToDevice, stream));
    const hipEvent_t e0 = o.kernel_ms ? d.mark() : nullptr;
    launch_stability(a, (int)G, stream);
    HIPCK(hipGetLastError());
    const hipEvent_t e1 = o.kernel_ms ? d.mark() : nullptr;
    if (o.kernel_ms && (!e0 || !e1)) return fail("event record failed");
    HIPCK(hipMemcpyAsync(o.assignments, a.assign, T * STAB_K * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCK(hipMemcpyAsync(abz.data(), a.a, abz.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipMemcpyAsync(o.consensus, a.consensus, G * STAB_K * VMAX * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipMemcpyAsync(o.cluster, a.cluster, G * STAB_K * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipMemcpyAsync(score.data(), a.score, score.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipMemcpyAsync(rounds.data(), a.rounds, rounds.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCK(hipStreamSynchronize(stream));
    std::copy(abz.begin(), abz.begin() + T * STAB_K, o.a);
    std::copy(abz.begin() + T * STAB_K, abz.begin() + 2 * T * STAB_K, o.b);
    std::copy(abz.begin() + 2 * T * STAB_K, abz.end(), o.silhouette);
    std::copy(score.begin(), score.end(), o.stability);
    for (size_t g = 0; g < G; ++g) {
        o.n_rounds[g] = rounds[2 * g];
        o.converged[g] = rounds[2 * g + 1];
    }
    if (o.kernel_ms) {
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, e0, e1));
        *o.kernel_ms = (double)ms;
    }
    return 0;
}

}  // namespace

extern "C" {

const char* salnmf_batch_last_error(void) { return g_err.c_str(); }

int salnmf_batch_create(int device, int n_features, int64_t n_samples, int n_members, const int* n_signatures, salnmf_batch** out) {
    if (!out) return fail("out is null");
    *out = nullptr;
    if (n_features < 1 || n_features > VMAX) return fail("n_features must be in [1, %d], got %d", VMAX, n_features);
    if (n_samples < 1 || n_samples > 16 * (int64_t)SMALL_MAX_TILES)
        return fail("n_samples must be in [1, %d], got %lld", 16 * SMALL_MAX_TILES, (long long)n_samples);
    if (n_members < 1 || !n_signatures) return fail("a batch needs at least one member");
    for (int m = 0; m < n_members; ++m)
        if (n_signatures[m] < 1 || n_signatures[m] > 16) return fail("member %d: n_signatures must be in [1, 16], got %d", m, n_signatures[m]);
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));

    salnmf_batch* b = new salnmf_batch();
    b->device = device;
    b->V = n_features;
    b->N = n_samples;
    b->M = n_members;
    b->ntiles = (n_samples + 15) / 16;
    b->Np = 16 * b->ntiles;
    b->fgrid = forward_grid(prop.multiProcessorCount, b->ntiles);
    b->K.assign(n_signatures, n_signatures + n_members);
    b->dataset.assign((size_t)n_members, -1);
    b->weights.assign((size_t)2 * n_members, nullptr);
    auto cleanup = [&](int rc) {
        salnmf_batch_destroy(b);
        return rc;
    };
    size_t kv = 0;
    for (int k : b->K) kv += (size_t)k * b->V;
    const size_t hsz = (size_t)b->Np * 16;
    const size_t state = 2 * kv + (size_t)b->M * hsz;  // W | G | H of every member
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) return cleanup(fail("stream create failed"));
    if (hipMalloc(&b->X, (size_t)b->Np * VMAX * sizeof(double)) != hipSuccess || hipMalloc(&b->xlx, (size_t)b->Np * 16 * sizeof(double)) != hipSuccess ||
        hipMalloc(&b->state, state * sizeof(double)) != hipSuccess || hipMalloc(&b->part, (size_t)b->M * b->fgrid * sizeof(double)) != hipSuccess ||
        hipMalloc(&b->klout, (size_t)b->M * b->Np * sizeof(double)) != hipSuccess || hipMalloc(&b->counter, (size_t)b->M * sizeof(unsigned)) != hipSuccess ||
        hipMalloc(&b->dmembers, (size_t)b->M * sizeof(BatchMember)) != hipSuccess || hipMalloc(&b->dstep, (size_t)2 * b->M * sizeof(int)) != hipSuccess ||
        hipMalloc(&b->dobj, (size_t)b->M * sizeof(int)) != hipSuccess || hipMalloc(&b->dweights, (size_t)2 * b->M * sizeof(double*)) != hipSuccess)
        return cleanup(fail("hipMalloc failed (batch of %d members)", n_members));
    if (hipHostMalloc(&b->pin, (size_t)SALNMF_BATCH_SLOTS * b->M * sizeof(double), hipHostMallocPortable) != hipSuccess)
        return cleanup(fail("hipHostMalloc failed"));
    b->ev.assign(SALNMF_BATCH_SLOTS, nullptr);
    b->queued.assign(SALNMF_BATCH_SLOTS, 0);
    for (auto& e : b->ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return cleanup(fail("event create failed"));
    double *W = b->state, *G = b->state + kv, *H = b->state + 2 * kv;
    for (int m = 0; m < n_members; ++m) {
        b->members.push_back(BatchMember{W, H, G, b->K[(size_t)m], b->X, b->xlx});
        W += (size_t)b->K[(size_t)m] * b->V;
        G += (size_t)b->K[(size_t)m] * b->V;
        H += hsz;
    }
    if (hipMemcpy(b->dmembers, b->members.data(), b->members.size() * sizeof(BatchMember), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(b->counter, 0, (size_t)b->M * sizeof(unsigned)) != hipSuccess || hipMemset(b->dweights, 0, (size_t)2 * b->M * sizeof(double*)) != hipSuccess || hipMemset(b->state, 0, state * sizeof(double)) != hipSuccess)
        return cleanup(fail("hipMemcpy failed"));
    *out = b;
    return 0;
}

void salnmf_batch_destroy(salnmf_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (hipEvent_t e : b->ev)
        if (e) (void)hipEventDestroy(e);
    for (void* p : {(void*)b->X, (void*)b->xlx, (void*)b->Xr, (void*)b->xlxr, (void*)b->state, (void*)b->part, (void*)b->klout, (void*)b->counter, (void*)b->dmembers, (void*)b->dstep,
                    (void*)b->dobj})
        if (p) (void)hipFree(p);
    for (double* w : b->weights)
        if (w) (void)hipFree(w);
    if (b->dweights) (void)hipFree(b->dweights);
    if (b->pin) (void)hipHostFree(b->pin);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int salnmf_batch_upload_X(salnmf_batch* b, const double* X, int clip) {
    if (!b || !X) return fail("null argument");
    HIPCK(hipSetDevice(b->device));
    // the engine's layout: pad rows and columns exactly 0 (never clipped), X.clip(EPSILON) as pad_rows_kernel does it
    std::vector<double> host((size_t)b->Np * VMAX, 0.0);
    for (int64_t n = 0; n < b->N; ++n)
        for (int v = 0; v < b->V; ++v) {
            double x = X[(size_t)n * b->V + v];
            if (clip) x = x < SALNMF_EPSILON ? SALNMF_EPSILON : x;
            host[(size_t)n * VMAX + v] = x;
        }
    HIPCK(hipStreamSynchronize(b->stream));
    drop_resamples(b);
    b->hostX.assign(X, X + (size_t)b->N * b->V);
    HIPCK(hipMemcpyAsync(b->X, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    launch_xlogx_lane(b->X, b->Np, b->V, b->xlx, b->stream);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(b->stream));
    b->x_ok = true;
    return 0;
}

int salnmf_batch_upload_member(salnmf_batch* b, int member, const double* W, const double* H) {
    CK(check_member(b, member));
    if (!W || !H) return fail("null argument");
    HIPCK(hipSetDevice(b->device));
    const BatchMember& mb = b->members[(size_t)member];
    const int K = mb.K;
    // H as salnmf_upload_H pads it for K <= 16: [Np][16], pad columns 0, pad rows 1 in the K columns (P > 0 there)
    std::vector<double> h((size_t)b->Np * 16);
    for (int64_t n = 0; n < b->Np; ++n)
        for (int k = 0; k < 16; ++k) h[(size_t)n * 16 + k] = k >= K ? 0.0 : n >= b->N ? 1.0 : H[(size_t)n * K + k];
    HIPCK(hipStreamSynchronize(b->stream));
    HIPCK(hipMemcpyAsync(mb.W, W, (size_t)K * b->V * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCK(hipMemcpyAsync(mb.H, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCK(hipStreamSynchronize(b->stream));
    return 0;
}

int salnmf_batch_download_member(salnmf_batch* b, int member, double* W, double* H) {
    CK(check_member(b, member));
    if (!W || !H) return fail("null argument");
    HIPCK(hipSetDevice(b->device));
    const BatchMember& mb = b->members[(size_t)member];
    const int K = mb.K;
    std::vector<double> h((size_t)b->N * 16);
    HIPCK(hipMemcpyAsync(W, mb.W, (size_t)K * b->V * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCK(hipMemcpyAsync(h.data(), mb.H, h.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCK(hipStreamSynchronize(b->stream));
    for (int64_t n = 0; n < b->N; ++n)
        for (int k = 0; k < K; ++k) H[(size_t)n * K + k] = h[(size_t)n * 16 + k];
    return 0;
}

int salnmf_batch_set_weights(salnmf_batch* b, int member, const double* weights_kl, const double* weights_lhalf) {
    CK(check_member(b, member));
    for (const double* w : {weights_kl, weights_lhalf})
        for (int64_t n = 0; w && n < b->N; ++n)
            if (!(w[n] >= 0.0) || !std::isfinite(w[n]))
                return fail("member %d: %s must be finite and non-negative, entry %lld is %g", member, w == weights_kl ? "weights_kl" : "weights_lhalf",
                            (long long)n, w[n]);
    HIPCK(hipSetDevice(b->device));
    HIPCK(hipStreamSynchronize(b->stream));  // (the launches that read the old arrays are done)
    auto set = [&](double*& dev, const double* host, double filler) -> int {
        if (!host) {
            double* old = dev;
            dev = nullptr;  // (first: a failing hipFree must not leave the pointer behind)
            if (old) HIPCK(hipFree(old));
            return 0;
        }
        if (!dev && hipMalloc(&dev, (size_t)b->Np * sizeof(double)) != hipSuccess) {
            dev = nullptr;
            return fail("hipMalloc failed (weights of member %d)", member);
        }
        std::vector<double> padded((size_t)b->Np, filler);  // as salnmf_set_weights pads an engine's
        std::copy(host, host + b->N, padded.begin());
        HIPCK(hipMemcpy(dev, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice));
        return 0;
    };
    // the member table follows in either case: a failure below leaves the member with the arrays it still has
    const int rc_kl = set(b->weights[(size_t)2 * member], weights_kl, 1.0);
    const int rc_lh = rc_kl ? rc_kl : set(b->weights[(size_t)2 * member + 1], weights_lhalf, 0.0);
    b->members_dirty = true;  // (the weight table is rewritten with the member table, like point_member's change)
    return rc_lh;
}

int salnmf_batch_kl_step(salnmf_batch* b, int n_steps, int n_active, const int* members, const int* n_given) {
    if (!b) return fail("null batch");
    CK(check_list(b, n_active, members));
    if (n_steps < 0) return fail("n_steps must not be negative");
    if (n_active == 0 || n_steps == 0) return 0;
    if (!b->x_ok) return fail("upload X first");
    if (!n_given) return fail("null n_given");
    HIPCK(hipSetDevice(b->device));
    for (int i = 0; i < n_active; ++i) {
        const int K = b->K[(size_t)members[i]];
        if (n_given[i] < 0 || n_given[i] >= K)
            return fail("member %d: n_given must be in [0, %d), got %d (all signatures given: nothing to step)", members[i], K, n_given[i]);
    }
    // the members without weights first (today's kernel), the weighted ones behind them (its weighted instantiation), each
    // part in the caller's order: [members | their n_given]
    auto weighted = [&](int m) { return b->weights[(size_t)2 * m] || b->weights[(size_t)2 * m + 1]; };
    std::vector<int> order;
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < n_active; ++i)
            if (weighted(members[i]) == (pass == 1)) order.push_back(i);
    int n_plain = 0;
    std::vector<int> want;
    for (int i : order) {
        want.push_back(members[i]);
        n_plain += !weighted(members[i]);
    }
    for (int i : order) want.push_back(n_given[i]);
    CK(set_list(b, b->dstep, b->step_list, want));
    CK(flush_members(b));
    SmallBatchArgs a{b->dmembers, b->dstep, b->dstep + n_active, b->V, (int)b->ntiles, 0, b->dweights};
    constexpr int kMaxPerLaunch = 4096;  // (salnmf_kl_step's bound on one launch of the small kernel)
    for (int i = 0; i < n_steps; i += a.nsteps) {
        a.nsteps = std::min(kMaxPerLaunch, n_steps - i);
        if (launch_small_kl_batch(a, n_plain, n_active - n_plain, b->stream)) return fail("no batched small-cohort kernel for %lld tiles", (long long)b->ntiles);
        HIPCK(hipGetLastError());
    }
    return 0;
}

int salnmf_batch_objective_async(salnmf_batch* b, int slot, int n_active, const int* members) {
    if (!b) return fail("null batch");
    if (slot < 0 || slot >= SALNMF_BATCH_SLOTS) return fail("slot must be in [0, %d)", SALNMF_BATCH_SLOTS);
    CK(check_list(b, n_active, members));
    if (!b->x_ok) return fail("upload X first");
    HIPCK(hipSetDevice(b->device));
    b->queued[(size_t)slot] = 1;
    if (n_active > 0) {
        CK(set_list(b, b->dobj, b->obj_list, std::vector<int>(members, members + n_active)));
        CK(flush_members(b));
        BatchFwdArgs a{b->dmembers, b->dobj, b->part, b->counter, b->pin + (size_t)slot * b->M, b->N, b->ntiles, b->V, nullptr, nullptr, b->dweights};
        hipLaunchKernelGGL(batch_forward_kernel<0>, dim3(b->fgrid, n_active), dim3(BLOCK), 0, b->stream, a);
        HIPCK(hipGetLastError());
    }
    HIPCK(hipEventRecord(b->ev[(size_t)slot], b->stream));
    return 0;
}

int salnmf_batch_objective_read(salnmf_batch* b, int first, int count, double* out) {
    if (!b || !out) return fail("null argument");
    if (first < 0 || count < 0 || first + count > SALNMF_BATCH_SLOTS) return fail("slots out of range");
    HIPCK(hipSetDevice(b->device));
    for (int s = first; s < first + count; ++s) {
        if (!b->queued[(size_t)s]) return fail("slot %d has never been queued", s);
        HIPCK(hipEventSynchronize(b->ev[(size_t)s]));
    }
    std::copy(b->pin + (size_t)first * b->M, b->pin + (size_t)(first + count) * b->M, out);
    return 0;
}

int salnmf_batch_samplewise_kl(salnmf_batch* b, double* out) {
    if (!b || !out) return fail("null argument");
    if (!b->x_ok) return fail("upload X first");
    HIPCK(hipSetDevice(b->device));
    std::vector<int> all((size_t)b->M);
    for (int m = 0; m < b->M; ++m) all[(size_t)m] = m;
    CK(set_list(b, b->dobj, b->obj_list, all));
    CK(flush_members(b));
    BatchFwdArgs a{b->dmembers, b->dobj, b->klout, nullptr, nullptr, b->N, b->ntiles, b->V};
    hipLaunchKernelGGL(batch_forward_kernel<1>, dim3(b->fgrid, b->M), dim3(BLOCK), 0, b->stream, a);
    HIPCK(hipGetLastError());
    std::vector<double> host((size_t)b->M * b->Np);
    HIPCK(hipMemcpyAsync(host.data(), b->klout, host.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCK(hipStreamSynchronize(b->stream));
    for (int m = 0; m < b->M; ++m) std::copy(host.begin() + (size_t)m * b->Np, host.begin() + (size_t)m * b->Np + b->N, out + (size_t)m * b->N);
    return 0;
}

int salnmf_batch_resample(salnmf_batch* b, int n_resamples, uint64_t seed) {
    if (!b) return fail("null batch");
    if (!b->x_ok) return fail("upload X first");
    CK(check_resample_args(n_resamples));
    if (b->F) return fail("this batch holds %d count splits: resamples and splits exclude each other on one batch (upload X again to drop them)", b->F);
    CK(draw_into_slots(b, n_resamples, batch_resample_launch(b, n_resamples, seed)));
    b->R = n_resamples;
    return 0;
}

int salnmf_batch_split(salnmf_batch* b, int n_splits, uint64_t thr, uint64_t seed) {
    if (!b) return fail("null batch");
    if (!b->x_ok) return fail("upload X first");
    CK(check_split_args(n_splits, thr));
    if (b->R && !b->F) return fail("this batch holds %d resamples: resamples and splits exclude each other on one batch (upload X again to drop them)", b->R);
    CK(draw_into_slots(b, 2 * n_splits, batch_split_launch(b, n_splits, thr, seed)));
    b->R = 2 * n_splits;
    b->F = n_splits;
    return 0;
}

int salnmf_batch_heldout_kl(salnmf_batch* b, int n_members, const int* members, const int* datasets, double scale, double* out) {
    if (!b) return fail("null batch");
    if (!out || !datasets) return fail("null argument");
    CK(check_list(b, n_members, members));
    if (n_members < 1) return fail("held-out scoring needs at least one member");
    if (!b->x_ok) return fail("upload X first");
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail("the exposure scale must be positive and finite, got %g", scale);
    // (host buffers of the asynchronous copies: declared before d, so they outlive its wait for the stream)
    std::vector<const double*> xs((size_t)n_members);
    for (int i = 0; i < n_members; ++i) {
        CK(check_dataset(b, datasets[i]));
        xs[(size_t)i] = dataset_ptr(b, datasets[i]);
    }
    const std::vector<double> hs(16, scale);
    std::vector<double> host((size_t)b->M * b->Np);
    HIPCK(hipSetDevice(b->device));
    CK(set_list(b, b->dobj, b->obj_list, std::vector<int>(members, members + n_members)));
    CK(flush_members(b));
    DevBufs d(b->stream);
    const double** dxs = d.get<const double*>(xs.size());
    double* dhs = d.get<double>(hs.size());
    if (!dxs || !dhs) return fail("hipMalloc failed (held-out scoring of %d members)", n_members);
    HIPCK(hipMemcpyAsync(dxs, xs.data(), xs.size() * sizeof(double*), hipMemcpyHostToDevice, b->stream));
    HIPCK(hipMemcpyAsync(dhs, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    BatchFwdArgs a{b->dmembers, b->dobj, b->klout, nullptr, nullptr, b->N, b->ntiles, b->V, dxs, dhs};
    hipLaunchKernelGGL(batch_forward_kernel<1>, dim3(b->fgrid, n_members), dim3(BLOCK), 0, b->stream, a);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(host.data(), b->klout, host.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCK(hipStreamSynchronize(b->stream));
    for (int i = 0; i < n_members; ++i) {
        const double* src = host.data() + (size_t)members[i] * b->Np;
        std::copy(src, src + b->N, out + (size_t)i * b->N);
    }
    return 0;
}

int salnmf_batch_set_dataset(salnmf_batch* b, int member, int dataset) {
    CK(check_member(b, member));
    CK(check_dataset(b, dataset));
    if (b->dataset[(size_t)member] != dataset) point_member(b, member, dataset);
    return 0;
}

int salnmf_batch_download_dataset(salnmf_batch* b, int dataset, int raw, double* out) {
    if (!b || !out) return fail("null argument");
    if (!b->x_ok) return fail("upload X first");
    CK(check_dataset(b, dataset));
    HIPCK(hipSetDevice(b->device));
    const double* src = dataset_ptr(b, dataset);
    if (raw) {
        HIPCK(hipMemcpyAsync(out, src, (size_t)b->Np * VMAX * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        HIPCK(hipStreamSynchronize(b->stream));
        return 0;
    }
    std::vector<double> host((size_t)b->N * VMAX);
    HIPCK(hipMemcpyAsync(host.data(), src, host.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCK(hipStreamSynchronize(b->stream));
    for (int64_t n = 0; n < b->N; ++n)
        for (int v = 0; v < b->V; ++v) {
            const double x = host[(size_t)n * VMAX + v];
            out[(size_t)n * b->V + v] = dataset >= 0 && x < 0.5 ? 0.0 : x;  // (a resample holds max(count, EPSILON))
        }
    return 0;
}

int salnmf_resample_counts(int device, const double* X, int64_t n_samples, int n_features, int n_resamples, uint64_t seed, double* out) {
    if (!X || !out) return fail("null argument");
    CK(check_resample_args(n_resamples));
    return draw_stand_alone(device, X, n_samples, n_features, n_resamples, out, nullptr, [=](const uint32_t* dcounts, double* dout) {
        launch_resample(ResampleArgs{dcounts, dout, n_samples, n_samples, n_features, n_features, (uint32_t)seed, (uint32_t)(seed >> 32), 0.0}, n_resamples, nullptr);
    });
}

int salnmf_split_counts(int device, const double* X, int64_t n_samples, int n_features, int n_splits, uint64_t thr, uint64_t seed, double* train_out,
                        double* test_out) {
    if (!X || !train_out || !test_out) return fail("null argument");
    CK(check_split_args(n_splits, thr));
    return draw_stand_alone(device, X, n_samples, n_features, n_splits, train_out, test_out, [=](const uint32_t* dcounts, double* dout) {
        double* test = dout + (size_t)n_splits * n_samples * n_features;
        launch_split(SplitArgs{dcounts, dout, test, n_samples, n_samples, n_features, n_features, (uint32_t)seed, (uint32_t)(seed >> 32), thr, 0.0}, n_splits, nullptr);
    });
}

int salnmf_profile_split(salnmf_batch* b, int n_splits, uint64_t thr, uint64_t seed, int n_calls, double* avg_ms) {
    return profile_draw(b, n_calls, avg_ms, [=] { return salnmf_batch_split(b, n_splits, thr, seed); }, batch_split_launch(b, n_splits, thr, seed));
}

int salnmf_profile_resample(salnmf_batch* b, int n_resamples, uint64_t seed, int n_calls, double* avg_ms) {
    return profile_draw(b, n_calls, avg_ms, [=] { return salnmf_batch_resample(b, n_resamples, seed); }, batch_resample_launch(b, n_resamples, seed));
}

int salnmf_batch_stability(salnmf_batch* b, int n_groups, const int* group_offsets, const int* members, const double* errors, int max_rounds,
                           int* assignments, int* n_rounds, int* converged, double* consensus, double* a, double* b_dist, double* silhouette,
                           double* cluster_stability, double* stability, double* kernel_ms) {
    if (!b) return fail("null batch");
    const StabOut o{assignments, n_rounds, converged, consensus, a, b_dist, silhouette, cluster_stability, stability, kernel_ms};
    CK(check_stab_out(o));
    if (n_groups < 1 || !group_offsets || !members) return fail("stability needs at least one group");
    if (max_rounds < 1) return fail("max_rounds must be positive, got %d", max_rounds);
    if (group_offsets[0] != 0) return fail("group_offsets must start at 0");
    if (b->V < 1 || b->V > VMAX) return fail("n_features must be in [1, %d], got %d", VMAX, b->V);
    std::vector<StabGroup> groups;
    std::vector<const double*> src;
    for (int g = 0; g < n_groups; ++g) {
        const int first = group_offsets[g], M = group_offsets[g + 1] - first;
        if (M < 0) return fail("group_offsets must not decrease (group %d)", g);
        for (int i = first; i < first + M; ++i) CK(check_member(b, members[i]));
        const int K = M > 0 ? b->K[(size_t)members[first]] : 1;
        CK(check_stab_group(g, K, M));
        for (int i = first; i < first + M; ++i) {
            if (b->K[(size_t)members[i]] != K)
                return fail("group %d mixes members of %d and %d signatures (members %d and %d)", g, K, b->K[(size_t)members[i]], members[first], members[i]);
            src.push_back(b->members[(size_t)members[i]].W);
        }
        groups.push_back(StabGroup{K, M, first});
    }
    HIPCK(hipSetDevice(b->device));
    return run_stability(b->stream, groups, src, b->V, b->V, errors, max_rounds, o);
}

int salnmf_signature_stability(int device, const double* signatures, int n_groups, const int* n_signatures, const int* n_members, int n_features,
                               const double* errors, int max_rounds, int* assignments, int* n_rounds, int* converged, double* consensus, double* a,
                               double* b_dist, double* silhouette, double* cluster_stability, double* stability, double* kernel_ms) {
    const StabOut o{assignments, n_rounds, converged, consensus, a, b_dist, silhouette, cluster_stability, stability, kernel_ms};
    CK(check_stab_out(o));
    if (!signatures || n_groups < 1 || !n_signatures || !n_members) return fail("stability needs at least one group");
    if (n_features < 1 || n_features > VMAX) return fail("n_features must be in [1, %d], got %d", VMAX, n_features);
    if (max_rounds < 1) return fail("max_rounds must be positive, got %d", max_rounds);
    std::vector<StabGroup> groups;
    size_t T = 0;
    for (int g = 0; g < n_groups; ++g) {
        CK(check_stab_group(g, n_signatures[g], n_members[g]));
        for (int m = 0; m < n_members[g]; ++m)
            for (int k = 0; k < n_signatures[g]; ++k) {
                const double* row = signatures + ((T + (size_t)m) * STAB_K + (size_t)k) * VMAX;
                double ss = 0.0;
                for (int v = 0; v < n_features; ++v) ss += row[v] * row[v];
                if (!std::isfinite(ss) || !(ss > 0.0))
                    return fail("group %d, member %d, signature %d: every signature needs finite entries and a positive norm", g, m, k);
            }
        groups.push_back(StabGroup{n_signatures[g], n_members[g], (int)T});
        T += (size_t)n_members[g];
    }
    hipDeviceProp_t prop;
    CK(open_device(device, &prop));
    DevBufs d;
    const size_t n = T * STAB_K * VMAX;
    double* dsig = d.get<double>(n);
    if (!dsig) return fail("hipMalloc failed (%zu signature matrices)", T);
    HIPCK(hipMemcpy(dsig, signatures, n * sizeof(double), hipMemcpyHostToDevice));
    std::vector<const double*> src(T);
    for (size_t t = 0; t < T; ++t) src[t] = dsig + t * STAB_K * VMAX;
    return run_stability(nullptr, groups, src, VMAX, n_features, errors, max_rounds, o);
}

}  // extern "C"
