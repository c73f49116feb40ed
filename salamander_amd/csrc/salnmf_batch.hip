// KLNMFSweep on the device: the batch handle of include/salnmf.h (salnmf_batch_*), the batched objective / per-sample
// divergence passes, and the host side of the batched step (its kernel: salnmf_small.hip, small_kl_batch_kernel).
// Layout and the bit-for-bit argument: salnmf_batch.h, DESIGN.md section 12.
#define SALNMF_TEMPLATES_ONLY 1
#include "../../include/salnmf.h"
#include "salnmf_batch.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

using namespace salnmf;

namespace salnmf {
namespace {

// one launch of the batched forward pass: blockIdx.y = entry of `active`, blockIdx.x = the workgroup of that member's
// pass (gridDim.x = the engine's fgrid for this shape)
struct BatchFwdArgs {
    const double* __restrict__ X;
    const double* __restrict__ xlx;     // [Np][16] (mode 0)
    const BatchMember* __restrict__ members;
    const int* __restrict__ active;
    double* part;                       // mode 0: [n_members][gridDim.x] workgroup partials
    unsigned* counter;                  // mode 0: [n_members] arrival counters, zero between launches
    double* sum_out;                    // mode 0: row `slot` of the objective array, [n_members] (pinned host memory)
    double* kl_out;                     // mode 1: [n_members][Np]
    int64_t N, Np, ntiles;
    int V;
};

template <int KS>
constexpr int bfwd_lds_doubles() { return 4 * KS * WS + WAVES * Geo<KS>::HL + BLOCK + Geo<KS>::KP + LOGTAB_DOUBLES; }

// forward_kernel<KS, MODE> (salnmf_forward_kernel.h) for one member, unweighted, no pending exposure scale, one feature
// block, one signature chunk -- what an engine of <= 16 signatures and <= 96 features runs for salnmf_objective_async (mode 0,
// the in-launch sum) and salnmf_samplewise_kl (mode 1).  The same statements in the same order: the same bits.
template <int KS, int MODE>
__device__ __forceinline__ void batch_forward_body(const BatchFwdArgs& a, const BatchMember& b, int m, double* lds) {
    using G_ = Geo<KS>;
    constexpr int KP = G_::KP, LS = G_::LS, HV = G_::HV;
    constexpr int FROWS = 4 * KS;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int c16 = lane & 15;
    const int q = lane >> 4;
    const int V = a.V, K = b.K;
    const int64_t N = a.N;

    double* Wl = lds;
    double* Hl = lds + FROWS * WS + wave * G_::HL;
    double* red = lds + FROWS * WS + WAVES * G_::HL;
    double* hsl = red + BLOCK;
    double* ltab = hsl + KP;
    if (MODE == 0) stage_logtab(ltab, tid);

    stage_W<FROWS>(Wl, b.W, K, V, V, tid);
    __syncthreads();

    int hrow[HV], hcol[HV];
#pragma unroll
    for (int j = 0; j < HV; ++j) {
        int e = 2 * lane + 128 * j;
        hrow[j] = e / KP;
        hcol[j] = e - hrow[j] * KP;
    }

    const int64_t tstride = (int64_t)gridDim.x * WAVES;
    double total = 0.0;

    for (int64_t tile = (int64_t)blockIdx.x * WAVES + wave; tile < a.ntiles; tile += tstride) {
        const int64_t n0 = tile * 16;
        const d2* hsrc = reinterpret_cast<const d2*>(b.H + n0 * KP) + lane;
        d2 hv[HV];
#pragma unroll
        for (int j = 0; j < HV; ++j) hv[j] = hsrc[64 * j];
        d4 pr[VT];
#pragma unroll
        for (int vt = 0; vt < VT; ++vt) pr[vt] = (d4){0, 0, 0, 0};
        double x[VT][4];
        {
            const double* xsrc = a.X + (n0 + q) * VMAX + c16;
#pragma unroll
            for (int vt = 0; vt < VT; ++vt)
#pragma unroll
                for (int r = 0; r < 4; ++r) x[vt][r] = xsrc[4 * r * VMAX + 16 * vt];
        }
        double wv[4] = {1.0, 1.0, 1.0, 1.0}, cv[4] = {0.0, 0.0, 0.0, 0.0};
        if (MODE == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) cv[r] = a.xlx[(n0 + q + 4 * r) * 16 + c16];
        }
        double pen = 0.0;
#pragma unroll
        for (int j = 0; j < HV; ++j) *reinterpret_cast<d2*>(Hl + hrow[j] * LS + hcol[j]) = hv[j];
        __builtin_amdgcn_wave_barrier();

        const double* ha = Hl + c16 * LS + q;
        const double* wb = Wl + q * WS + c16;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            double av = ha[4 * s];
#pragma unroll
            for (int vt = 0; vt < VT; ++vt) pr[vt] = mfma(av, wb[4 * s * WS + 16 * vt], pr[vt]);
        }

        if (MODE == 0) {
            total += pen + tile_kl<true>(x, pr, wv, cv, ltab, n0, N, V, q, c16);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int64_t n = n0 + q + 4 * r;
                double acc = 0.0;
#pragma unroll
                for (int vt = 0; vt < VT; ++vt)
                    if (n < N && 16 * vt + c16 < V) {
                        double xv = x[vt][r], pv = pr[vt][r];
                        double xe = (xv == 0.0) ? kEps : xv, pe = (xv == 0.0) ? kEps : pv;
                        double l = (log_operand_ok(xe) && log_operand_ok(pe)) ? log_ratio(xe, pe) : log(xe / pe);
                        acc += xe * l - xv + pv;
                    }
#pragma unroll
                for (int mm = 1; mm < 16; mm <<= 1) acc += __shfl_xor(acc, mm, 64);
                if (c16 == 0) a.kl_out[(int64_t)m * a.Np + n] = acc;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }

    if (MODE == 0) {
        double* out = a.part + (size_t)m * gridDim.x;
        unsigned* counter = a.counter + m;
        red[tid] = total;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < BLOCK; ++i) s += red[i];
            __hip_atomic_store((gdouble*)(out + blockIdx.x), s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned ticket = __hip_atomic_fetch_add((gsync_t*)counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            red[0] = (ticket == gridDim.x - 1u) ? 1.0 : 0.0;
        }
        __syncthreads();
        const bool last = red[0] != 0.0;  // (uniform)
        __syncthreads();
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            double sum = 0.0;
            for (int i = tid; i < (int)gridDim.x; i += BLOCK) sum += ld_shared<true>(out + i);
            red[tid] = sum;
            __syncthreads();
            for (int h = BLOCK / 2; h > 0; h >>= 1) {
                if (tid < h) red[tid] += red[tid + h];
                __syncthreads();
            }
            if (tid == 0) {
                a.sum_out[m] = red[0];
                __hip_atomic_store((gsync_t*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// members of 1-4, 5-8 and 9-16 signatures share the launch (forward_kernel's geometries KS = 1, 2, 4; the branch is
// uniform per workgroup, LDS is sized for the widest)
template <int MODE>
__global__ void __launch_bounds__(BLOCK, 2) batch_forward_kernel(BatchFwdArgs a) {
    static_assert(bfwd_lds_doubles<4>() * 8 <= 80 * 1024, "two workgroups per CU, as forward_kernel at KS <= 4");
    __shared__ __attribute__((aligned(16))) double lds[bfwd_lds_doubles<4>()];
    const int m = a.active[blockIdx.y];
    const BatchMember& b = a.members[m];
    if (b.K <= 4)
        batch_forward_body<1, MODE>(a, b, m, lds);
    else if (b.K <= 8)
        batch_forward_body<2, MODE>(a, b, m, lds);
    else
        batch_forward_body<4, MODE>(a, b, m, lds);
}

// xlogx_lane_kernel (salnmf_plain_kernels.h), restated: that kernel is compiled into salnmf.hip only
__global__ void __launch_bounds__(256) batch_xlogx_kernel(const double* __restrict__ X, int64_t Np, int V, double* __restrict__ c) {
    const int64_t n = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    if (n >= Np) return;
    double s = 0.0;
    for (int v = l; v < V; v += 16) s += kl_term_x(X[n * VMAX + v]);
    c[n * 16 + l] = s;
}

}  // namespace
}  // namespace salnmf

struct salnmf_batch {
    int device = 0, V = 0, M = 0;
    int64_t N = 0, Np = 0, ntiles = 0;
    int fgrid = 0;  // workgroups of an engine's forward pass at this shape (salnmf_create): the objective's summation order
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
};

static thread_local std::string g_batch_err;

static int bfail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_batch_err = buf;
    return 1;
}

#define BHIPCK(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return bfail("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define BCK(call)              \
    do {                       \
        int rc_ = (call);      \
        if (rc_) return rc_;   \
    } while (0)

static int check_member(const salnmf_batch* b, int m) {
    if (!b) return bfail("null batch");
    if (m < 0 || m >= b->M) return bfail("member %d out of range (%d members)", m, b->M);
    return 0;
}

// a list of n member indices, each in range and none twice
static int check_list(const salnmf_batch* b, int n, const int* members) {
    if (n < 0 || n > b->M) return bfail("%d members listed, the batch has %d", n, b->M);
    if (n > 0 && !members) return bfail("null member list");
    std::vector<char> seen((size_t)b->M, 0);
    for (int i = 0; i < n; ++i) {
        BCK(check_member(b, members[i]));
        if (seen[(size_t)members[i]]++) return bfail("member %d listed twice", members[i]);
    }
    return 0;
}

// a device list is rewritten only when it changes -- after the host has read objectives and dropped converged members --
// and only once the launches that read its old content are done
static int set_list(salnmf_batch* b, int* dev, std::vector<int>& cache, const std::vector<int>& want) {
    if (cache == want) return 0;
    BHIPCK(hipStreamSynchronize(b->stream));
    BHIPCK(hipMemcpy(dev, want.data(), want.size() * sizeof(int), hipMemcpyHostToDevice));
    cache = want;
    return 0;
}

extern "C" {

const char* salnmf_batch_last_error(void) { return g_batch_err.c_str(); }

int salnmf_batch_create(int device, int n_features, int64_t n_samples, int n_members, const int* n_signatures, salnmf_batch** out) {
    if (!out) return bfail("out is null");
    *out = nullptr;
    if (n_features < 1 || n_features > VMAX) return bfail("n_features must be in [1, %d], got %d", VMAX, n_features);
    if (n_samples < 1 || n_samples > 16 * (int64_t)SMALL_MAX_TILES)
        return bfail("n_samples must be in [1, %d], got %lld", 16 * SMALL_MAX_TILES, (long long)n_samples);
    if (n_members < 1 || !n_signatures) return bfail("a batch needs at least one member");
    for (int m = 0; m < n_members; ++m)
        if (n_signatures[m] < 1 || n_signatures[m] > 16) return bfail("member %d: n_signatures must be in [1, 16], got %d", m, n_signatures[m]);
    int ndev = 0;
    BHIPCK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return bfail("device %d out of range (%d visible)", device, ndev);
    BHIPCK(hipSetDevice(device));
    hipDeviceProp_t prop;
    BHIPCK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) return bfail("this build targets gfx950 only; device %d is %s", device, prop.gcnArchName);

    salnmf_batch* b = new salnmf_batch();
    b->device = device;
    b->V = n_features;
    b->N = n_samples;
    b->M = n_members;
    b->ntiles = (n_samples + 15) / 16;
    b->Np = 16 * b->ntiles;
    b->fgrid = (int)std::min<int64_t>(2 * prop.multiProcessorCount, (b->ntiles + WAVES - 1) / WAVES);
    b->K.assign(n_signatures, n_signatures + n_members);
    auto cleanup = [&](int rc) {
        salnmf_batch_destroy(b);
        return rc;
    };
    size_t kv = 0;
    for (int k : b->K) kv += (size_t)k * b->V;
    const size_t hsz = (size_t)b->Np * 16;
    const size_t state = 2 * kv + (size_t)b->M * hsz;  // W | G | H of every member
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) return cleanup(bfail("stream create failed"));
    if (hipMalloc(&b->X, (size_t)b->Np * VMAX * sizeof(double)) != hipSuccess || hipMalloc(&b->xlx, (size_t)b->Np * 16 * sizeof(double)) != hipSuccess ||
        hipMalloc(&b->state, state * sizeof(double)) != hipSuccess || hipMalloc(&b->part, (size_t)b->M * b->fgrid * sizeof(double)) != hipSuccess ||
        hipMalloc(&b->klout, (size_t)b->M * b->Np * sizeof(double)) != hipSuccess || hipMalloc(&b->counter, (size_t)b->M * sizeof(unsigned)) != hipSuccess ||
        hipMalloc(&b->dmembers, (size_t)b->M * sizeof(BatchMember)) != hipSuccess || hipMalloc(&b->dstep, (size_t)2 * b->M * sizeof(int)) != hipSuccess ||
        hipMalloc(&b->dobj, (size_t)b->M * sizeof(int)) != hipSuccess)
        return cleanup(bfail("hipMalloc failed (batch of %d members)", n_members));
    if (hipHostMalloc(&b->pin, (size_t)SALNMF_BATCH_SLOTS * b->M * sizeof(double), hipHostMallocPortable) != hipSuccess)
        return cleanup(bfail("hipHostMalloc failed"));
    b->ev.assign(SALNMF_BATCH_SLOTS, nullptr);
    b->queued.assign(SALNMF_BATCH_SLOTS, 0);
    for (auto& e : b->ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return cleanup(bfail("event create failed"));
    double *W = b->state, *G = b->state + kv, *H = b->state + 2 * kv;
    for (int m = 0; m < n_members; ++m) {
        b->members.push_back(BatchMember{W, H, G, b->K[(size_t)m]});
        W += (size_t)b->K[(size_t)m] * b->V;
        G += (size_t)b->K[(size_t)m] * b->V;
        H += hsz;
    }
    if (hipMemcpy(b->dmembers, b->members.data(), b->members.size() * sizeof(BatchMember), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(b->counter, 0, (size_t)b->M * sizeof(unsigned)) != hipSuccess || hipMemset(b->state, 0, state * sizeof(double)) != hipSuccess)
        return cleanup(bfail("hipMemcpy failed"));
    *out = b;
    return 0;
}

void salnmf_batch_destroy(salnmf_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (hipEvent_t e : b->ev)
        if (e) (void)hipEventDestroy(e);
    for (void* p : {(void*)b->X, (void*)b->xlx, (void*)b->state, (void*)b->part, (void*)b->klout, (void*)b->counter, (void*)b->dmembers, (void*)b->dstep,
                    (void*)b->dobj})
        if (p) (void)hipFree(p);
    if (b->pin) (void)hipHostFree(b->pin);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

int salnmf_batch_upload_X(salnmf_batch* b, const double* X, int clip) {
    if (!b || !X) return bfail("null argument");
    BHIPCK(hipSetDevice(b->device));
    // the engine's layout: pad rows and columns exactly 0 (never clipped), X.clip(EPSILON) as pad_rows_kernel does it
    std::vector<double> host((size_t)b->Np * VMAX, 0.0);
    for (int64_t n = 0; n < b->N; ++n)
        for (int v = 0; v < b->V; ++v) {
            double x = X[(size_t)n * b->V + v];
            if (clip) x = x < SALNMF_EPSILON ? SALNMF_EPSILON : x;
            host[(size_t)n * VMAX + v] = x;
        }
    BHIPCK(hipStreamSynchronize(b->stream));
    BHIPCK(hipMemcpyAsync(b->X, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    hipLaunchKernelGGL(batch_xlogx_kernel, dim3((unsigned)((b->Np + 15) / 16)), dim3(256), 0, b->stream, b->X, b->Np, b->V, b->xlx);
    BHIPCK(hipGetLastError());
    BHIPCK(hipStreamSynchronize(b->stream));
    b->x_ok = true;
    return 0;
}

int salnmf_batch_upload_member(salnmf_batch* b, int member, const double* W, const double* H) {
    BCK(check_member(b, member));
    if (!W || !H) return bfail("null argument");
    BHIPCK(hipSetDevice(b->device));
    const BatchMember& mb = b->members[(size_t)member];
    const int K = mb.K;
    // H as salnmf_upload_H pads it for K <= 16: [Np][16], pad columns 0, pad rows 1 in the K columns (P > 0 there)
    std::vector<double> h((size_t)b->Np * 16);
    for (int64_t n = 0; n < b->Np; ++n)
        for (int k = 0; k < 16; ++k) h[(size_t)n * 16 + k] = k >= K ? 0.0 : n >= b->N ? 1.0 : H[(size_t)n * K + k];
    BHIPCK(hipStreamSynchronize(b->stream));
    BHIPCK(hipMemcpyAsync(mb.W, W, (size_t)K * b->V * sizeof(double), hipMemcpyHostToDevice, b->stream));
    BHIPCK(hipMemcpyAsync(mb.H, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    BHIPCK(hipStreamSynchronize(b->stream));
    return 0;
}

int salnmf_batch_download_member(salnmf_batch* b, int member, double* W, double* H) {
    BCK(check_member(b, member));
    if (!W || !H) return bfail("null argument");
    BHIPCK(hipSetDevice(b->device));
    const BatchMember& mb = b->members[(size_t)member];
    const int K = mb.K;
    std::vector<double> h((size_t)b->N * 16);
    BHIPCK(hipMemcpyAsync(W, mb.W, (size_t)K * b->V * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    BHIPCK(hipMemcpyAsync(h.data(), mb.H, h.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    BHIPCK(hipStreamSynchronize(b->stream));
    for (int64_t n = 0; n < b->N; ++n)
        for (int k = 0; k < K; ++k) H[(size_t)n * K + k] = h[(size_t)n * 16 + k];
    return 0;
}

int salnmf_batch_kl_step(salnmf_batch* b, int n_steps, int n_active, const int* members, const int* n_given) {
    if (!b) return bfail("null batch");
    BCK(check_list(b, n_active, members));
    if (n_steps < 0) return bfail("n_steps must not be negative");
    if (n_active == 0 || n_steps == 0) return 0;
    if (!b->x_ok) return bfail("upload X first");
    if (!n_given) return bfail("null n_given");
    BHIPCK(hipSetDevice(b->device));
    std::vector<int> want(members, members + n_active);
    for (int i = 0; i < n_active; ++i) {
        const int K = b->K[(size_t)members[i]];
        if (n_given[i] < 0 || n_given[i] >= K)
            return bfail("member %d: n_given must be in [0, %d), got %d (all signatures given: nothing to step)", members[i], K, n_given[i]);
        want.push_back(n_given[i]);
    }
    BCK(set_list(b, b->dstep, b->step_list, want));
    SmallBatchArgs a{b->X, b->dmembers, b->dstep, b->dstep + n_active, b->V, (int)b->ntiles, 0};
    constexpr int kMaxPerLaunch = 4096;  // (salnmf_kl_step's bound on one launch of the small kernel)
    for (int i = 0; i < n_steps; i += a.nsteps) {
        a.nsteps = std::min(kMaxPerLaunch, n_steps - i);
        if (launch_small_kl_batch(a, n_active, b->stream)) return bfail("no batched small-cohort kernel for %lld tiles", (long long)b->ntiles);
        BHIPCK(hipGetLastError());
    }
    return 0;
}

int salnmf_batch_objective_async(salnmf_batch* b, int slot, int n_active, const int* members) {
    if (!b) return bfail("null batch");
    if (slot < 0 || slot >= SALNMF_BATCH_SLOTS) return bfail("slot must be in [0, %d)", SALNMF_BATCH_SLOTS);
    BCK(check_list(b, n_active, members));
    if (!b->x_ok) return bfail("upload X first");
    BHIPCK(hipSetDevice(b->device));
    b->queued[(size_t)slot] = 1;
    if (n_active > 0) {
        BCK(set_list(b, b->dobj, b->obj_list, std::vector<int>(members, members + n_active)));
        BatchFwdArgs a{b->X, b->xlx, b->dmembers, b->dobj, b->part, b->counter, b->pin + (size_t)slot * b->M, nullptr, b->N, b->Np, b->ntiles, b->V};
        hipLaunchKernelGGL(batch_forward_kernel<0>, dim3(b->fgrid, n_active), dim3(BLOCK), 0, b->stream, a);
        BHIPCK(hipGetLastError());
    }
    BHIPCK(hipEventRecord(b->ev[(size_t)slot], b->stream));
    return 0;
}

int salnmf_batch_objective_read(salnmf_batch* b, int first, int count, double* out) {
    if (!b || !out) return bfail("null argument");
    if (first < 0 || count < 0 || first + count > SALNMF_BATCH_SLOTS) return bfail("slots out of range");
    BHIPCK(hipSetDevice(b->device));
    for (int s = first; s < first + count; ++s) {
        if (!b->queued[(size_t)s]) return bfail("slot %d has never been queued", s);
        BHIPCK(hipEventSynchronize(b->ev[(size_t)s]));
    }
    std::copy(b->pin + (size_t)first * b->M, b->pin + (size_t)(first + count) * b->M, out);
    return 0;
}

int salnmf_batch_samplewise_kl(salnmf_batch* b, double* out) {
    if (!b || !out) return bfail("null argument");
    if (!b->x_ok) return bfail("upload X first");
    BHIPCK(hipSetDevice(b->device));
    std::vector<int> all((size_t)b->M);
    for (int m = 0; m < b->M; ++m) all[(size_t)m] = m;
    BCK(set_list(b, b->dobj, b->obj_list, all));
    BatchFwdArgs a{b->X, b->xlx, b->dmembers, b->dobj, nullptr, nullptr, nullptr, b->klout, b->N, b->Np, b->ntiles, b->V};
    hipLaunchKernelGGL(batch_forward_kernel<1>, dim3(b->fgrid, b->M), dim3(BLOCK), 0, b->stream, a);
    BHIPCK(hipGetLastError());
    std::vector<double> host((size_t)b->M * b->Np);
    BHIPCK(hipMemcpyAsync(host.data(), b->klout, host.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    BHIPCK(hipStreamSynchronize(b->stream));
    for (int m = 0; m < b->M; ++m) std::copy(host.begin() + (size_t)m * b->Np, host.begin() + (size_t)m * b->Np + b->N, out + (size_t)m * b->N);
    return 0;
}

}  // extern "C"
