// Count splitting (Poisson thinning) of a count matrix, drawn on the device (include/salnmf.h: salnmf_split_counts,
// salnmf_batch_split).
//
// Every single mutation of row n goes to the training matrix with probability p = thr / 2^64, independently of all others:
//   mutation j of the row (0 <= j < T_n) belongs to cell v(j) = the smallest v with cum[v] > j, cum the row's inclusive
//   integer prefix sums;
//   Philox4x32-10 (salnmf_resample.h: philox4x32_10), key = (seed & 0xffffffff, seed >> 32);
//   block q of row n of split f has counter (q, 0x53504C54, n, f) -- the resampler's second counter word is always 0, so
//   the two streams never meet under one seed -- and gives the words (o0, o1, o2, o3);
//   draw 2q uses u = o0 | o1 << 32, draw 2q + 1 uses u = o2 | o3 << 32, draws j >= T_n are discarded;
//   mutation j goes to train iff u_j < thr.
// train[n, v] counts the mutations of cell v sent to train and test[n, v] = X[n, v] - train[n, v].  For Poisson counts of
// mean lambda the two halves are independent Poisson counts of means p lambda and (1 - p) lambda.
// Everything is integer arithmetic and the histogram is a sum of ones: the result does not depend on which lane performs
// which draw or on the order of the atomic adds, and split f does not depend on how many splits are drawn.
#pragma once
#include "salnmf_resample.h"

namespace salnmf {

constexpr uint32_t SPLIT_STREAM = 0x53504C54u;  // "SPLT": the second counter word of every block of this stream

struct SplitArgs {
    const uint32_t* __restrict__ counts;  // [N][V] the observed counts
    double* __restrict__ train;           // [F][rows_out][ld]
    double* __restrict__ test;            // [F][rows_out][ld]
    int64_t N, rows_out;                  // rows_out >= N: rows beyond N are written as zeros
    int V, ld;                            // ld >= V: columns beyond V are written as zeros
    uint32_t key0, key1;
    uint64_t thr;                         // a mutation goes to train iff its 64-bit draw is below thr
    double floor;                         // entries of the N x V blocks are max(count, floor): 0 (raw) or SALNMF_EPSILON
};

// the cell of mutation j < cum[V - 1]: the smallest v with cum[v] > j
__device__ __forceinline__ int split_cell(uint32_t j, const uint32_t* cum, int V) {
    int lo = 0, hi = V - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > j)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// One workgroup per (output row, split): blockIdx.x = row, blockIdx.y = split.  LDS as resample_counts_kernel: the prefix
// sums and one histogram (train); test is x - train at write-out.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) split_counts_kernel(SplitArgs a) {
    __shared__ uint32_t cum[RESAMPLE_VMAX];
    __shared__ uint32_t hist[RESAMPLE_VMAX];
    __shared__ uint32_t part[RESAMPLE_BLOCK];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x;
    const uint32_t f = blockIdx.y;
    const size_t row = ((size_t)f * a.rows_out + n) * a.ld;
    double* train = a.train + row;
    double* test = a.test + row;
    if (n >= a.N) {  // a pad row of the batch layout
        for (int v = tid; v < a.ld; v += RESAMPLE_BLOCK) train[v] = test[v] = 0.0;
        return;
    }
    const int V = a.V;
    const uint32_t* x = a.counts + (size_t)n * V;
    for (int v = tid; v < V; v += RESAMPLE_BLOCK) {
        cum[v] = x[v];
        hist[v] = 0;
    }
    __syncthreads();
    // inclusive prefix sums, as the resampler builds them: every lane scans its own stretch, the stretches' totals are
    // scanned across the workgroup, and every lane adds the total of the stretches before its own
    const int chunk = (V + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK;
    const int first = min(tid * chunk, V), last = min(first + chunk, V);
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
    // T draws, two per Philox block; lanes stride over the blocks (T < 2^32: the block index fits 32 bits)
    const uint32_t nblocks = (T >> 1) + (T & 1);
    for (uint32_t q = tid; q < nblocks; q += RESAMPLE_BLOCK) {
        uint32_t o[4];
        philox4x32_10(q, SPLIT_STREAM, (uint32_t)n, f, a.key0, a.key1, o);
        const uint32_t j = 2u * q;  // (j + 1 <= T - 1 < 2^32 where it is used)
        if (((uint64_t)o[1] << 32 | o[0]) < a.thr) atomicAdd(&hist[split_cell(j, cum, V)], 1u);
        if (2 * (uint64_t)q + 1 < T && ((uint64_t)o[3] << 32 | o[2]) < a.thr) atomicAdd(&hist[split_cell(j + 1u, cum, V)], 1u);
    }
    __syncthreads();
    for (int v = tid; v < a.ld; v += RESAMPLE_BLOCK) {
        double tr = 0.0, te = 0.0;
        if (v < V) {
            const uint32_t h = hist[v];
            tr = (double)h;
            te = (double)(x[v] - h);
            tr = tr < a.floor ? a.floor : tr;
            te = te < a.floor ? a.floor : te;
        }
        train[v] = tr;
        test[v] = te;
    }
}

inline void launch_split(const SplitArgs& a, int n_splits, hipStream_t stream) {
    hipLaunchKernelGGL(split_counts_kernel, dim3((unsigned)a.rows_out, (unsigned)n_splits), dim3(RESAMPLE_BLOCK), 0, stream, a);
}

}  // namespace salnmf
