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

// the split's draw: mutation j stays in its own cell, and is counted (sent to train) iff its draw is below thr
struct SplitDraw {
    static constexpr uint32_t stream = SPLIT_STREAM;
    uint32_t index;  // the split
    uint64_t thr;
    double *train, *test;  // its rows
    __device__ int place(uint32_t j, uint32_t ulo, uint32_t uhi, uint32_t, const uint32_t* cum, int V) const {
        return ((uint64_t)uhi << 32 | ulo) < thr ? upper_cell(j, cum, V) : -1;
    }
    __device__ void write_row(int tid, int ld, int V, double floor, const uint32_t* x, const uint32_t* hist) const {
        for (int v = tid; v < ld; v += RESAMPLE_BLOCK) {
            double tr = 0.0, te = 0.0;
            if (v < V) {
                tr = clipped_count(hist[v], floor);
                te = clipped_count(x[v] - hist[v], floor);
            }
            train[v] = tr;
            test[v] = te;
        }
    }
};

// One workgroup per (output row, split): blockIdx.x = row, blockIdx.y = split.  The histogram of count_draw_row is train;
// test is x - train at write-out.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) split_counts_kernel(SplitArgs a) {
    const size_t row = ((size_t)blockIdx.y * a.rows_out + blockIdx.x) * a.ld;
    const SplitDraw d{blockIdx.y, a.thr, a.train + row, a.test + row};
    count_draw_row(a.counts, a.N, a.V, a.ld, a.key0, a.key1, a.floor, d);
}

inline void launch_split(const SplitArgs& a, int n_splits, hipStream_t stream) {
    hipLaunchKernelGGL(split_counts_kernel, dim3((unsigned)a.rows_out, (unsigned)n_splits), dim3(RESAMPLE_BLOCK), 0, stream, a);
}

}  // namespace salnmf
