// Bootstrap resamples of a count matrix, drawn on the device (include/salnmf.h: salnmf_resample_counts,
// salnmf_batch_resample; DESIGN.md section 12, "Resampling").
//
// Row n of resample r is one multinomial draw of T_n = sum_v X[n, v] trials with probabilities X[n, :] / T_n, built as T_n
// categorical draws from a counter-based generator:
//   Philox4x32-10 (Salmon et al., Random123), key = (seed & 0xffffffff, seed >> 32);
//   block q of row n of resample r has counter (q mod 2^32, q >> 32, n, r) and gives the words (o0, o1, o2, o3);
//   draw 2q uses u = o0 | o1 << 32, draw 2q + 1 uses u = o2 | o3 << 32, draws j >= T_n are discarded;
//   t = floor(u T_n / 2^64) (T_n < 2^32), and the draw lands in the smallest v with cum[v] > t, cum the integer prefix sums.
// Everything is integer arithmetic and the histogram is a sum of ones: the result does not depend on which lane performs
// which draw or on the order of the atomic adds, and resample r does not depend on how many resamples are drawn.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace salnmf {

constexpr int RESAMPLE_VMAX = 3072;   // the project's n_features limit: prefix sums and histogram, 2 x 12 KB of LDS
constexpr int RESAMPLE_BLOCK = 256;

struct ResampleArgs {
    const uint32_t* __restrict__ counts;  // [N][V] the observed counts
    double* __restrict__ out;             // [R][rows_out][ld]
    int64_t N, rows_out;                  // rows_out >= N: rows beyond N are written as zeros
    int V, ld;                            // ld >= V: columns beyond V are written as zeros
    uint32_t key0, key1;
    double floor;                         // entries of the N x V block are max(count, floor): 0 (raw) or SALNMF_EPSILON
    uint32_t first;                       // slot 0 of `out` holds resample `first` (a chunk of a longer series: salnmf_refit.h)
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o[0] = c0, o[1] = c1, o[2] = c2, o[3] = c3;
}

// the bin of one draw: t = high 64 bits of u * T (T < 2^32, so t < T fits 32 bits), then the smallest v with cum[v] > t
__device__ __forceinline__ int resample_bin(uint32_t ulo, uint32_t uhi, uint32_t T, const uint32_t* cum, int V) {
    const uint64_t low = (uint64_t)ulo * T;
    const uint32_t t = (uint32_t)(((uint64_t)uhi * T + (low >> 32)) >> 32);
    int lo = 0, hi = V - 1;  // cum[V - 1] = T > t: the answer is in [0, V - 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// One workgroup per (output row, resample): blockIdx.x = row, blockIdx.y = resample.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) resample_counts_kernel(ResampleArgs a) {
    __shared__ uint32_t cum[RESAMPLE_VMAX];
    __shared__ uint32_t hist[RESAMPLE_VMAX];
    __shared__ uint32_t part[RESAMPLE_BLOCK];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x;
    const uint32_t r = blockIdx.y + a.first;
    double* out = a.out + ((size_t)blockIdx.y * a.rows_out + n) * a.ld;
    if (n >= a.N) {  // a pad row of the batch layout
        for (int v = tid; v < a.ld; v += RESAMPLE_BLOCK) out[v] = 0.0;
        return;
    }
    const int V = a.V;
    const uint32_t* x = a.counts + (size_t)n * V;
    for (int v = tid; v < V; v += RESAMPLE_BLOCK) {
        cum[v] = x[v];
        hist[v] = 0;
    }
    __syncthreads();
    // inclusive prefix sums: every lane scans its own stretch of `chunk` entries, the stretches' totals are scanned across
    // the workgroup, and every lane adds the total of the stretches before its own
    const int chunk = (V + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK;
    const int first = tid * chunk, last = min(first + chunk, V);
    uint32_t sum = 0;
    for (int v = first; v < last; ++v) cum[v] = sum += cum[v];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < RESAMPLE_BLOCK; d <<= 1) {
        const uint32_t add = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const uint32_t before = tid ? part[tid - 1] : 0;
    for (int v = first; v < last; ++v) cum[v] += before;
    __syncthreads();
    const uint32_t T = cum[V - 1];
    // T draws, two per Philox block; lanes stride over the blocks (T < 2^32: the block index fits 32 bits, q >> 32 is 0)
    const uint32_t nblocks = (T >> 1) + (T & 1);
    for (uint32_t q = tid; q < nblocks; q += RESAMPLE_BLOCK) {
        uint32_t o[4];
        philox4x32_10(q, 0u, (uint32_t)n, r, a.key0, a.key1, o);
        atomicAdd(&hist[resample_bin(o[0], o[1], T, cum, V)], 1u);
        if (2 * (uint64_t)q + 1 < T) atomicAdd(&hist[resample_bin(o[2], o[3], T, cum, V)], 1u);
    }
    __syncthreads();
    for (int v = tid; v < a.ld; v += RESAMPLE_BLOCK) {
        double c = 0.0;
        if (v < V) {
            c = (double)hist[v];
            c = c < a.floor ? a.floor : c;
        }
        out[v] = c;
    }
}

inline void launch_resample(const ResampleArgs& a, int n_resamples, hipStream_t stream) {
    hipLaunchKernelGGL(resample_counts_kernel, dim3((unsigned)a.rows_out, (unsigned)n_resamples), dim3(RESAMPLE_BLOCK), 0, stream, a);
}

}  // namespace salnmf
