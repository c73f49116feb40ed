// Goodness of fit of a sample to a catalogue by parametric bootstrap (include/salnmf.h: salnmf_draw_model_counts,
// salnmf_goodness_of_fit): count vectors drawn on the device from a sample's FITTED model, and the
// reduction of the null refits' divergences to a count of exceedances.
//
// Row n of draw b is one multinomial draw of T_n trials from the spectrum of exposures h (K doubles) under signatures W (K x V):
//   P_v = sum_k h_k W[k, v], from 0.0 in ascending k, every term a rounded product followed by a rounded sum (no fused
//   multiply-add);  S = sum_v P_v, from 0.0 in ascending v.  With S == 0, S not finite or T_n == 0 the row has no draws;
//   m_v = (uint64) floor((P_v / S) 2^40), the division correctly rounded, the power of two exact, the conversion truncating;
//   cum_v the 64-bit inclusive prefix sums of m, M = cum_{V-1} (M <= V 2^40 < 2^47);
//   Philox4x32-10 (salnmf_resample.h: philox4x32_10), key = (seed & 0xffffffff, seed >> 32);
//   block q of row n of draw b has counter (q, 0x474F4644, n, b) -- the resampler's second counter word is always 0 and the
//   split's 0x53504C54, so the three streams never meet under one seed; the presence test's draws (salnmf_presence.h) use
//   0x50530000 + s, a fourth family -- and gives the words (o0, o1, o2, o3);
//   draw 2q uses u = o0 | o1 << 32, draw 2q + 1 uses u = o2 | o3 << 32, draws j >= T_n are discarded;
//   t = floor(u M / 2^64) (the high 64 bits of the 128-bit product), and the draw lands in the smallest v with cum_v > t.
// After the weights everything is integer arithmetic and the histogram is a sum of ones: the result does not depend on which
// lane performs which draw or on the order of the atomic adds, and draw b does not depend on how many draws are made.
//
// The table is this kernel's own, not count_draw_row's: that one is 32 bits wide, built from integer counts, and takes its
// trial count from the table's total; here the weights carry 40 bits each (a 32-bit table of 96 cells would leave a cell 25
// bits) and the trial count comes from the sample.
// The refits of the observed counts and of the draws are refit_kernel launches (salnmf_refit.h, built from its solve_* pieces); the
// host driver is gof_run (salnmf_refit_drivers.h), which the negative-binomial test shares.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace salnmf {

constexpr uint32_t GOF_STREAM = 0x474F4644u;  // "GOFD": the second counter word of every block of this stream
constexpr int GOF_VMAX = 96;                  // the refit's limits: n_features and n_signatures
constexpr int GOF_KMAX = 96;
constexpr int GOF_MAX_DRAWS = 65536;
constexpr int GOF_GRID_Y = 32768;  // draws per launch (the draw is the grid's y)

struct ModelDrawArgs {
    const double* __restrict__ H;         // [N][K] the exposures
    const double* __restrict__ W;         // [K][V] the signatures, rows of sum one
    const uint32_t* __restrict__ totals;  // [N] the trial counts, or null: then row n's is sum_v (uint32) X[n, v]
    const double* __restrict__ X;         // [N][V] integer counts, zeros possibly clipped to a floor below 1 (read with totals == null)
    double* __restrict__ out;             // [draws][N][V]
    int64_t N;
    int V, K;
    uint32_t key0, key1;
    double floor;    // entries are max(count, floor): 0 (raw) or SALNMF_EPSILON
    uint32_t first;  // slot 0 of `out` holds draw `first`
};

struct GofReduceArgs {
    const double* __restrict__ err_obs;   // [N] the observed refit's divergences
    const double* __restrict__ err_null;  // [B][N] the null refits'
    int* __restrict__ n_exceed;           // [N]
    double* __restrict__ null_mean;       // [N]
    int64_t N;
    int B;
};

// salnmf_batch.hip (the translation unit that includes salnmf_resample.h, whose kernel one unit alone may define): draws
// first .. first + count - 1 of the series of `seed` as out[count][N][V], and the reduction
void gof_launch_model_draw(const double* H, const double* W, const uint32_t* totals, const double* X, double* out, int64_t N, int V, int K,
                           uint64_t seed, double floor, int first, int count, hipStream_t stream);
void gof_launch_reduce(const GofReduceArgs& a, hipStream_t stream);

#ifdef SALNMF_GOF_KERNELS  // salnmf_batch.hip alone compiles the kernels (it includes salnmf_resample.h first)

// the cell of position t < cum[V - 1]: the smallest v with cum[v] > t (upper_cell of salnmf_resample.h on a 64-bit table)
__device__ __forceinline__ int upper_cell64(uint64_t t, const uint64_t* cum, int V) {
    int lo = 0, hi = V - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// acc + a b with the product rounded before the sum.  (The toolchain's __dmul_rn / __dadd_rn are the plain operators, which the
// default contraction mode may still fuse once they are inlined: the pragma is what rules the fused form out.)
__device__ __forceinline__ double mul_then_add(double acc, double a, double b) {
#pragma clang fp contract(off)
    const double prod = a * b;
    return acc + prod;
}

// Row n of draw b by one workgroup, the body of every model draw: the exposures h (K), the stream word and the output row are
// the caller's.  The trial count is *total, or with total == null sum_v (uint32) xrow[v].
__device__ __forceinline__ void model_draw_row(const double* __restrict__ h, const double* __restrict__ W, const uint32_t* __restrict__ total,
                                               const double* __restrict__ xrow, double* __restrict__ out, int V, int K, uint32_t key0, uint32_t key1,
                                               uint32_t stream, uint32_t n, uint32_t b, double floor) {
    __shared__ double hs[GOF_KMAX];
    __shared__ double P[GOF_VMAX];
    __shared__ uint64_t cum[GOF_VMAX];
    __shared__ uint32_t hist[GOF_VMAX];
    __shared__ uint32_t trials;
    const int tid = threadIdx.x;
    if (tid < K) hs[tid] = h[tid];
    if (tid < V) hist[tid] = 0;
    __syncthreads();
    if (tid < V) {
        double p = 0.0;
        for (int k = 0; k < K; ++k) p = mul_then_add(p, hs[k], W[k * V + tid]);
        P[tid] = p;
    }
    __syncthreads();
    if (tid == 0) {  // the sum and the table in one fixed order
        double S = 0.0;
        for (int v = 0; v < V; ++v) S += P[v];
        uint32_t T = 0;
        if (total)
            T = *total;
        else
            for (int v = 0; v < V; ++v) T += (uint32_t)xrow[v];
        if (!(S > 0.0) || !(S < __builtin_inf())) T = 0;
        if (T) {
            uint64_t c = 0;
            for (int v = 0; v < V; ++v) cum[v] = c += (uint64_t)(__ddiv_rn(P[v], S) * 0x1p40);
        }
        trials = T;
    }
    __syncthreads();
    const uint32_t T = trials;
    if (T) {
        const uint64_t M = cum[V - 1];
        // T draws, two per Philox block; lanes stride over the blocks (T < 2^32: the block index fits 32 bits)
        const uint32_t nblocks = (T >> 1) + (T & 1);
        for (uint32_t q = tid; q < nblocks; q += RESAMPLE_BLOCK) {
            uint32_t o[4];
            philox4x32_10(q, stream, n, b, key0, key1, o);
            atomicAdd(&hist[upper_cell64(__umul64hi((uint64_t)o[1] << 32 | o[0], M), cum, V)], 1u);
            if (2 * (uint64_t)q + 1 < T) atomicAdd(&hist[upper_cell64(__umul64hi((uint64_t)o[3] << 32 | o[2], M), cum, V)], 1u);
        }
    }
    __syncthreads();
    if (tid < V) out[tid] = clipped_count(hist[tid], floor);
}

// One workgroup per (row, draw): blockIdx.x = row, blockIdx.y = draw - a.first.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) model_draw_kernel(ModelDrawArgs a) {
    const int64_t n = blockIdx.x;
    model_draw_row(a.H + (size_t)n * a.K, a.W, a.totals ? a.totals + n : nullptr, a.X + (size_t)n * a.V, a.out + ((size_t)blockIdx.y * a.N + n) * a.V,
                   a.V, a.K, a.key0, a.key1, GOF_STREAM, (uint32_t)n, blockIdx.y + a.first, a.floor);
}

// One thread per sample: the null divergences at or above the observed one, counted in ascending b (a NaN on either side
// compares false), and their mean -- the sum from 0.0 in ascending b, divided by B.
__global__ void __launch_bounds__(256) gof_reduce_kernel(GofReduceArgs a) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= a.N) return;
    const double obs = a.err_obs[n];
    int count = 0;
    double sum = 0.0;
    for (int b = 0; b < a.B; ++b) {
        const double e = a.err_null[(size_t)b * a.N + n];
        count += e >= obs ? 1 : 0;
        sum += e;
    }
    a.n_exceed[n] = count;
    a.null_mean[n] = sum / (double)a.B;
}
#endif  // SALNMF_GOF_KERNELS

}  // namespace salnmf
