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

// the cell of position t < cum[V - 1]: the smallest v with cum[v] > t
__device__ __forceinline__ int upper_cell(uint32_t t, const uint32_t* cum, int V) {
    int lo = 0, hi = V - 1;  // cum[V - 1] > t: the answer is in [0, V - 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ double clipped_count(uint32_t c, double floor) { return (double)c < floor ? floor : (double)c; }

// One row of one draw, by one workgroup of RESAMPLE_BLOCK lanes: everything the count-drawing kernels share.  Row n of
// `counts` ([N][V]) is loaded, its T_n trials are drawn two per Philox block, and the row is written out `ld` cells wide
// (ld >= V; a row n >= N is a pad row of the batch layout).  What tells one kind of draw from another is `Draw`, passed by value:
//   stream, index   the second and the fourth counter word of every block (the first is q, the third n);
//   place(j, ulo, uhi, T, cum, V)   the cell that trial j, with the 64-bit draw u = ulo | uhi << 32, adds one to, or -1 for none;
//   write_row(tid, ld, V, floor, x, hist)   the row from its counts x and the histogram of the placed trials: cells below V
//                   clipped to `floor`, cells from V on zero (a pad row is written with V = 0 and reads neither array).
template <typename Draw>
__device__ __forceinline__ void count_draw_row(const uint32_t* __restrict__ counts, int64_t N, int V, int ld, uint32_t key0, uint32_t key1, double floor,
                                               const Draw d) {
    __shared__ uint32_t cum[RESAMPLE_VMAX];
    __shared__ uint32_t hist[RESAMPLE_VMAX];
    __shared__ uint32_t part[RESAMPLE_BLOCK];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x;
    if (n >= N) {  // a pad row of the batch layout
        d.write_row(tid, ld, 0, floor, nullptr, nullptr);
        return;
    }
    const uint32_t* x = counts + (size_t)n * V;
    for (int v = tid; v < V; v += RESAMPLE_BLOCK) {
        cum[v] = x[v];
        hist[v] = 0;
    }
    __syncthreads();
    // inclusive prefix sums: every lane scans its own stretch of `chunk` entries, the stretches' totals are scanned across
    // the workgroup, and every lane adds the total of the stretches before its own
    const int chunk = (V + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK;
    const int first = min(tid * chunk, V), last = min(first + chunk, V);
    uint32_t sum = 0;
    for (int v = first; v < last; ++v) cum[v] = sum += cum[v];
    part[tid] = sum;
    __syncthreads();
    for (int s = 1; s < RESAMPLE_BLOCK; s <<= 1) {
        const uint32_t add = tid >= s ? part[tid - s] : 0;
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
        philox4x32_10(q, d.stream, (uint32_t)n, d.index, key0, key1, o);
        const uint32_t j = 2u * q;  // (j + 1 <= T - 1 < 2^32 where it is used)
        int cell = d.place(j, o[0], o[1], T, cum, V);
        if (cell >= 0) atomicAdd(&hist[cell], 1u);
        if (2 * (uint64_t)q + 1 < T) {
            cell = d.place(j + 1u, o[2], o[3], T, cum, V);
            if (cell >= 0) atomicAdd(&hist[cell], 1u);
        }
    }
    __syncthreads();
    d.write_row(tid, ld, V, floor, x, hist);
}

// the resampler's draw: trial j lands at position t = high 64 bits of u * T (T < 2^32, so t < T fits 32 bits)
struct ResampleDraw {
    static constexpr uint32_t stream = 0u;
    uint32_t index;  // the resample
    double* out;     // its row
    __device__ int place(uint32_t, uint32_t ulo, uint32_t uhi, uint32_t T, const uint32_t* cum, int V) const {
        const uint64_t low = (uint64_t)ulo * T;
        return upper_cell((uint32_t)(((uint64_t)uhi * T + (low >> 32)) >> 32), cum, V);
    }
    __device__ void write_row(int tid, int ld, int V, double floor, const uint32_t*, const uint32_t* hist) const {
        for (int v = tid; v < ld; v += RESAMPLE_BLOCK) out[v] = v < V ? clipped_count(hist[v], floor) : 0.0;
    }
};

// One workgroup per (output row, resample): blockIdx.x = row, blockIdx.y = resample.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) resample_counts_kernel(ResampleArgs a) {
    const ResampleDraw d{blockIdx.y + a.first, a.out + ((size_t)blockIdx.y * a.rows_out + blockIdx.x) * a.ld};
    count_draw_row(a.counts, a.N, a.V, a.ld, a.key0, a.key1, a.floor, d);
}

inline void launch_resample(const ResampleArgs& a, int n_resamples, hipStream_t stream) {
    hipLaunchKernelGGL(resample_counts_kernel, dim3((unsigned)a.rows_out, (unsigned)n_resamples), dim3(RESAMPLE_BLOCK), 0, stream, a);
}

}  // namespace salnmf
