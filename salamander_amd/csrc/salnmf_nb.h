// Negative-binomial refit of exposures to FIXED signatures (include/salnmf.h: salnmf_nb_refit_exposures).
//
// The refit family's problem (salnmf_refit.h) under another likelihood: a row's counts are negative binomial around p = h W with
// variance p + p^2 / alpha, the dispersion alpha > 0 a datum of the PROBLEM (alpha[P], read once per tile).  Contract:
//   x = max(row, EPSILON);  h_k = (sum_v x_v) / K;
//   step: p = h W, a_v = x_v / p_v, b_v = (x_v + alpha) / (p_v + alpha), h_k <- max((h_k sum_v W[k, v] a_v) / (sum_v W[k, v] b_v), EPSILON)
//   objective: sum_v [ x_v log(x_v / p_v) - (x_v + alpha) log((x_v + alpha) / (p_v + alpha)) ], >= 0, 0 at p = x, the KL divergence
//   as alpha -> infinity; evaluated, tested and latched exactly as refit_kernel does (iteration 0 and every multiple of
//   conv_test_freq, from the P^T just formed for the next step).
//
// nb_refit_kernel is refit_kernel's loop with one more product: the same transposed formulation (W the A operand from LDS, the
// wave's data the B operand straight from the accumulators, h never out of registers, one tile ticket per wave), and in the U
// phase TWO accumulator sets -- u_num takes a = div_path(x, p), u_den takes b = div_path(x + alpha, p + alpha) -- that consume the
// SAME W operand read, so the step's LDS traffic is refit_kernel's.  Pads: a and b are 0 in rows v >= V; u_den is 0 in the pad
// rows k >= K, where the quotient is never formed (the divisor is replaced by 1 there) and h stays 0 by selection.
// Built from salnmf_refit.h's pieces: solve_stage_w, solve_take_tile, solve_load_row, solve_store_column and solve_stop; the P^T
// product is kept in line as everywhere in the family.  All branches are wave-uniform; plain vector stores only.
#pragma once
#include "salnmf_refit.h"

namespace salnmf {

constexpr double NB_ALPHA_MAX = 1e6;  // beyond it the second logarithm's argument is 1 to rounding

struct NbRefitArgs {
    const double* __restrict__ X;      // [P][V] compact, clipped
    const double* __restrict__ W;      // [K][V]
    const double* __restrict__ alpha;  // [P]
    double* __restrict__ H;            // [P][K]
    double* __restrict__ err;          // [P]
    int* __restrict__ nit;             // [P]
    int* __restrict__ conv;            // [P]
    unsigned* next_tile;               // zero at launch: the tile list's head
    int64_t P;                         // problems
    int V, K;
    int min_it, max_it, freq;
    double tol;
};

#ifdef SALNMF_NB_KERNELS  // the units of the negative-binomial kernels (salnmf_kernels.h first, salnmf_refit.h's pieces enabled)

__device__ __forceinline__ double nb_log(double x, double p) {
    return (log_operand_ok(x) && log_operand_ok(p)) ? log_ratio(x, p) : log(x / p);
}

// One problem's NB divergence from the lane's 24 entries (rows v = 16 vt + 4 r + q of column c16): the lane's entries in (vt, r)
// order, then the four q groups by rows_sum -- the same bits in all four lanes of the column.
__device__ __forceinline__ double nb_objective(const double (&x)[VT][4], const d4 (&pr)[VT], double al, int V, int q) {
    double acc = 0.0;
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * vt + 4 * r + q < V) {
                const double xv = x[vt][r], pv = pr[vt][r];
                const double xa = xv + al, pa = pv + al;
                acc += xv * nb_log(xv, pv) - xa * nb_log(xa, pa);
            }
        asm volatile("" : "+v"(acc));  // one feature tile's logarithms at a time (refit_objective's reason)
    }
    return rows_sum(acc);
}

#ifndef SALNMF_NB_PIECES_ONLY  // salnmf_nb_assign.hip takes nb_log and nb_objective above and leaves the kernel to salnmf_nb.hip

template <int KT>
__global__ void __launch_bounds__(BLOCK) nb_refit_kernel(NbRefitArgs a) {
    constexpr int KP = 16 * KT;
    __shared__ double Wl[KP * WS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c16 = lane & 15, q = lane >> 4;
    const int V = a.V, K = a.K;
    solve_stage_w<KT>(Wl, a.W, K, V, tid);
    const int64_t ntiles = (a.P + 15) / 16;
    const double* wp = Wl + q * WS + c16;  // P^T: A[i = v][k] = W[4 s + q][16 vt + c16]
    const double* wu = Wl + c16 * WS + q;  // U^T: A[i = k][v] = W[16 kt + c16][4 s + q]

    for (;;) {
        const int64_t tile = solve_take_tile(a.next_tile, lane);
        if (tile >= ntiles) break;
        const int64_t p = tile * 16 + c16;
        const int64_t row = p < a.P ? p : a.P - 1;
        double x[VT][4];
        const double t = solve_load_row(a.X + row * V, V, q, x);
        const double al = a.alpha[row];
        d4 h[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[kt][r] = (16 * kt + 4 * r + q < K) ? t / (double)K : 0.0;

        bool latched = false;
        int nit = 0, conv = 0;
        double prev = 0.0, err = 0.0;
        int until_test = 0;  // steps until the next multiple of conv_test_freq
        for (int it = 0;; ++it) {
            d4 pr[VT];
#pragma unroll
            for (int vt = 0; vt < VT; ++vt) pr[vt] = (d4){0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4 * KT; ++s) {
                const double b = h[s >> 2][s & 3];
#pragma unroll
                for (int vt = 0; vt < VT; ++vt) pr[vt] = mfma(wp[4 * s * WS + 16 * vt], b, pr[vt]);
            }
            const bool at_test = until_test == 0;
            until_test = (at_test ? a.freq : until_test) - 1;
            if (at_test || it == a.max_it) {  // (uniform)
                const double cur = nb_objective(x, pr, al, V, q);
                if (!latched) {
                    // (refit_kernel's rule: the tolerance counts at a test iteration only; max_it need not be one)
                    int cv = 0;
                    const bool stop = at_test ? solve_stop(it, prev, cur, a.min_it, a.max_it, a.tol, cv) : it == a.max_it;
                    if (stop) latched = true, conv = cv;
                    prev = err = cur;
                    nit = it;
                }
                if (__all(latched)) break;
            }
            // U^T twice on one W operand stream: the numerator's factors a and the denominator's b
            d4 un[KT], ud[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) un[kt] = (d4){0, 0, 0, 0}, ud[kt] = (d4){0, 0, 0, 0};
#pragma unroll
            for (int vt = 0; vt < VT; ++vt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool in = 16 * vt + 4 * r + q < V;
                    const double av = in ? div_path(x[vt][r], pr[vt][r]) : 0.0;
                    const double bv = in ? div_path(x[vt][r] + al, pr[vt][r] + al) : 0.0;
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt) {
                        const double w = wu[16 * kt * WS + 4 * (4 * vt + r)];
                        un[kt] = mfma(w, av, un[kt]);
                        ud[kt] = mfma(w, bv, ud[kt]);
                    }
                }
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool pad = 16 * kt + 4 * r + q >= K;
                    // (in a pad row u_den is 0: the quotient there is taken over 1 and dropped, never 0 0 / 0)
                    const double hn = clip_lo(div_path(h[kt][r] * un[kt][r], pad ? 1.0 : ud[kt][r]), kEps);
                    h[kt][r] = (latched || pad) ? h[kt][r] : hn;
                }
        }
        if (p < a.P) {
            solve_store_column<KT>(a.H + p * K, h, K, q);
            if (q == 0) {
                a.err[p] = err;
                a.nit[p] = nit;
                a.conv[p] = conv;
            }
        }
    }
}
#endif  // SALNMF_NB_PIECES_ONLY
#endif  // SALNMF_NB_KERNELS

}  // namespace salnmf
