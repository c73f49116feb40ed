// Is signature s present in this sample?  A parametric-bootstrap p-value per (sample, tested signature) for a nested pair of
// fits (include/salnmf.h: salnmf_signature_presence).
//
// A PAIR is a sample n with candidate set C and a tested signature s in C, |C| >= 2; pairs with s outside C or C = {s} are
// untested and never reach the device.  A problem is a row x and a pair: the sample's own counts (the observed launch) or one
// null draw of the pair.  Its two SOLVES are those defined at the top of salnmf_assign.h, each from a cold start:
//   the alternative on C:        h_k = sum(x) / |C| on C, exactly 0.0 off it        -> f1 (and h1 for an observed row)
//   the null        on C \ {s}:  h_k = sum(x) / (|C| - 1) on C \ {s}, 0.0 off it    -> f0 (and h0 for an observed row)
// bit for bit what assign_kernel<KT, true> returns with candidates = required = the set; the statistic is t = f0 - f1.
//
// Null draw b of the pair (n, s) is the model draw of salnmf_gof.h, steps 1-6, from the spectrum h0 W with the sample's own
// total, under the Philox counter (q, 0x50530000 + s, n, b): the second word carries the stream family "PS" -- no other
// draw's word has these upper 16 bits (the resampler's is 0, the split's 0x53504C54, the goodness-of-fit draw's 0x474F4644) --
// and the tested signature, so a pair's draws depend on (seed, n, s, b) and on h0, and on nothing else.
//
// presence_kernel is refit_kernel's tile loop (the solve_* pieces of salnmf_refit.h) with assign_kernel's way of letting one solve follow another: max_iterations is a
// multiple of conv_test_freq, every solve ends at a test, and the columns whose alternative solve has just ended reset their
// start and run the loop body again from the P^T product without stepping -- the null solve's iteration-0 test.  x is loaded
// once for both solves.  Branches are taken on ballots, the transitions are predicated per column, and a column's numbers
// never meet another column's (salnmf_refit.h).  A draw problem leaves t and its two iteration counts; an observed problem
// also its two exposure rows, divergences and convergence flags.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace salnmf {

constexpr uint32_t PRESENCE_STREAM = 0x50530000u;  // "PS" << 16: the second counter word of a block is this plus the tested signature

struct PresenceArgs {
    const double* __restrict__ X;       // by_sample: [N][V], problem p reads row pair_n[p]; otherwise [P][V], problem p reads row p
    const double* __restrict__ W;       // [K][V]
    const int* __restrict__ pair_n;     // [NP] the sample of pair j; problem p belongs to pair p % NP
    const int* __restrict__ pair_s;     // [NP] its tested signature
    const unsigned* __restrict__ cand;  // [N][NW] candidate words of sample n, NW = (KT + 1) / 2; or null: all K
    double* __restrict__ stat;          // [P] f0 - f1
    int* __restrict__ nit;              // [P][2] iterations of the alternative and of the null solve
    double* __restrict__ f;             // [P][2] f1, f0;                       observed launch, else null
    int* __restrict__ conv;             // [P][2]                                with f
    double* __restrict__ H1;            // [P][K] the alternative's exposures    with f
    double* __restrict__ H0;            // [P][K] the null's                     with f
    unsigned* next_tile;                // zero at launch
    int64_t P, NP;
    int V, K, by_sample;
    int min_it, max_it, freq;  // max_it % freq == 0
    double tol;
};

struct PresenceDrawArgs {
    const double* __restrict__ H0;   // [NP][K] the null fit's exposures of every pair, where the observed launch left them
    const double* __restrict__ W;    // [K][V]
    const double* __restrict__ X;    // [N][V] the clipped counts: row n's trial count is sum_v (uint32) X[n, v]
    const int* __restrict__ pair_n;  // [NP]
    const int* __restrict__ pair_s;  // [NP]
    double* __restrict__ out;        // [draws][NP][V]
    int64_t NP;
    int V, K;
    uint32_t key0, key1;
    double floor;
    uint32_t first;  // slot 0 of `out` holds draw `first`
};

// salnmf_batch.hip (the translation unit of model_draw_kernel): draws first .. first + count - 1 of every pair as out[count][NP][V]
void presence_launch_draw(const double* H0, const double* W, const double* X, const int* pair_n, const int* pair_s, double* out, int64_t NP, int V,
                          int K, uint64_t seed, double floor, int first, int count, hipStream_t stream);

#ifdef SALNMF_GOF_KERNELS  // salnmf_batch.hip: after salnmf_gof.h
// One workgroup per (pair, draw): model_draw_kernel's body with the exposure row and the stream word of the pair.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) presence_draw_kernel(PresenceDrawArgs a) {
    const int64_t j = blockIdx.x;
    const int n = a.pair_n[j], s = a.pair_s[j];
    model_draw_row(a.H0 + (size_t)j * a.K, a.W, nullptr, a.X + (size_t)n * a.V, a.out + ((size_t)blockIdx.y * a.NP + j) * a.V, a.V, a.K, a.key0,
                   a.key1, PRESENCE_STREAM + (uint32_t)s, (uint32_t)n, blockIdx.y + a.first, a.floor);
}
#endif  // SALNMF_GOF_KERNELS

#ifdef SALNMF_REFIT_KERNELS  // salnmf_refit.hip: after salnmf_assign.h
template <int KT>
__global__ void __launch_bounds__(BLOCK) presence_kernel(PresenceArgs a) {
    constexpr int KP = 16 * KT;
    constexpr int NW = (KT + 1) / 2;  // 32-bit words of a signature set
    __shared__ double Wl[KP * WS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c16 = lane & 15, q = lane >> 4;
    const int V = a.V, K = a.K;
    solve_stage_w<KT>(Wl, a.W, K, V, tid);
    const int64_t ntiles = (a.P + 15) / 16;
    const double* wp = Wl + q * WS + c16;
    const double* wu = Wl + c16 * WS + q;

    for (;;) {
        const int64_t tile = solve_take_tile(a.next_tile, lane);
        if (tile >= ntiles) break;
        const int64_t p = tile * 16 + c16;
        const int64_t row = p < a.P ? p : a.P - 1;
        const int64_t pair = row % a.NP;
        const int n = a.pair_n[pair], s = a.pair_s[pair];
        double x[VT][4];
        const double t = solve_load_row(a.X + (a.by_sample ? (int64_t)n : row) * V, V, q, x);
        // the column's set, the same in its four lanes: C for the first solve, C \ {s} for the second.  A lane column past the
        // end of the list is finished from the start: it recomputes the last problem's first step and touches no memory.
        unsigned act[NW];
        const int nc = solve_candidate_words<NW>(K, a.cand, (int64_t)n * NW, act);
        d4 h[KT];
        auto start = [&](int members) {
            const double h0 = t / (double)members;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) h[kt][r] = ((act[kt >> 1] >> ((16 * kt + 4 * r + q) & 31)) & 1u) ? h0 : 0.0;
        };
        start(nc);
        int mode = p < a.P ? 0 : 2;  // 0: the solve on C, 1: the solve on C \ {s}, 2: finished
        bool fresh = false;          // the solve has just started: its iteration-0 test is due
        int itl = 0;
        double prev = 0.0, f1 = 0.0;
        auto latch = [&](double* H, int which, double cur, int cv) {  // (the caller's predicate holds)
            if (H) solve_store_column<KT>(H + p * K, h, K, q);
            if (q == 0) {
                a.nit[2 * p + which] = itl;
                if (a.f) a.f[2 * p + which] = cur, a.conv[2 * p + which] = cv;
            }
        };

        int until_test = 0;   // steps until the next multiple of conv_test_freq (uniform)
        bool repass = false;  // this pass of the body follows a transition without a step (uniform)
        for (;;) {
            d4 pr[VT];
#pragma unroll
            for (int vt = 0; vt < VT; ++vt) pr[vt] = (d4){0, 0, 0, 0};
#pragma unroll
            for (int st = 0; st < 4 * KT; ++st) {
                const double b = h[st >> 2][st & 3];
#pragma unroll
                for (int vt = 0; vt < VT; ++vt) pr[vt] = mfma(wp[4 * st * WS + 16 * vt], b, pr[vt]);
            }
            if (until_test == 0) {  // (uniform)
                const double cur = refit_objective(x, pr, V, q);
                bool stop = false;
                int cv = 0;
                if (mode != 2 && (fresh || !repass)) {
                    stop = solve_stop(itl, prev, cur, a.min_it, a.max_it, a.tol, cv);
                    prev = cur;
                }
                fresh = false;
                if (__any(stop)) {
                    if (stop && mode == 1) {
                        latch(a.H0, 1, cur, cv);
                        if (q == 0) a.stat[p] = cur - f1;
                        mode = 2;
                    }
                    if (stop && mode == 0) {
                        latch(a.H1, 0, cur, cv);
                        f1 = cur;
#pragma unroll
                        for (int w = 0; w < NW; ++w) act[w] &= ~((s >> 5) == w ? 1u << (s & 31) : 0u);
                        start(nc - 1);
                        mode = 1, itl = 0, fresh = true;
                    }
                }
                if (__all(mode == 2)) break;
                if (__any(fresh)) {
                    repass = true;
                    continue;
                }
                repass = false;
                until_test = a.freq;
            }
            --until_test;
            d4 u[KT];
            solve_update_factors<KT>(x, pr, wu, V, q, u);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double hn = clip_lo(h[kt][r] * u[kt][r], kEps);
                    h[kt][r] = (mode == 2 || h[kt][r] == 0.0) ? h[kt][r] : hn;
                }
            ++itl;
        }
    }
}
#endif  // SALNMF_REFIT_KERNELS

}  // namespace salnmf
