// Is signature s present in this sample, under the negative-binomial model?  salnmf_presence.h's test with section 23's step
// and divergence and section 24's draw (include/salnmf.h: salnmf_nb_signature_presence).
//
// A PAIR, a problem and its two SOLVES are salnmf_presence.h's; a solve is salnmf_nb_assign.h's: the negative-binomial step
// on the entries that are not 0.0 (the product first, then one division, the divisor replaced by 1 in the pad rows k >= K),
// tests by solve_stop on nb_objective at iteration 0 and at every multiple of conv_test_freq.  Each solve is bit for bit what
// nb_assign_kernel returns with candidates = required = the set; the statistic is t = f0 - f1 at the sample's alpha.
//
// Null draw b of the pair (n, s) is salnmf_nbdraw.h's gamma-Poisson draw from the exposures h0 with alpha_n -- UNCONDITIONAL:
// its total varies -- through nb_draw_row unchanged, with row word n and draw word ((s + 1) << 16) | b.  b < 65 536 fills the
// low half-word and s + 1 <= 96 the next bits, so no two (s, b) share a word, and none is a word of salnmf_draw_nb_counts or
// salnmf_nb_goodness_of_fit, whose upper half-word is 0.  A pair's draws depend on (seed, n, s, b), h0 and alpha_n only.
//
// nb_presence_kernel is presence_kernel statement for statement around the negative-binomial step and objective; alpha is
// read once per tile as alpha[pair_n[pair]].  The U phase is nb_update_factors (salnmf_nb_assign.h): un for every k-tile, then ud
// one k-tile at a time behind the fence.  nb_refit_kernel's side-by-side form fits at KT <= 5 but leaves 28 bytes of scratch per
// lane at KT = 6; this one has none at any KT, and both are the same MFMA chains in ascending (vt, r), so the bits are the same.
// Plain vector stores only; every branch is wave-uniform; no synchronisation beyond the tile ticket.
#pragma once
#include "salnmf_nb.h"
#include "salnmf_nb_assign.h"
#include "salnmf_nbdraw.h"
#include "salnmf_presence.h"

namespace salnmf {

struct NbPresenceArgs : PresenceArgs {
    const double* __restrict__ alpha;  // [N]: a problem of pair j reads alpha[pair_n[j]]
};

struct NbPresenceDrawArgs {
    const double* __restrict__ H0;     // [NP][K] the null fit's exposures of every pair, where the observed launch left them
    const double* __restrict__ W;      // [K][V]
    const double* __restrict__ alpha;  // [N] the dispersions, and the gamma draw's constants of salnmf_nbdraw.h
    const double* __restrict__ gd;     // [N]
    const double* __restrict__ gc;     // [N]
    const int* __restrict__ pair_n;    // [NP]
    const int* __restrict__ pair_s;    // [NP]
    double* __restrict__ out;          // [draws][NP][V]
    unsigned* failed;                  // one word: rows written as zeros (salnmf_nbdraw.h)
    int64_t NP;
    int V, K;
    uint32_t key0, key1;
    double floor;
    uint32_t first;  // slot 0 of `out` holds draw `first`
};

// salnmf_batch.hip (the translation unit of nb_draw_kernel): draws first .. first + count - 1 of every pair as out[count][NP][V]
void nb_presence_launch_draw(const double* H0, const double* W, const double* alpha, const double* gd, const double* gc, const int* pair_n,
                             const int* pair_s, double* out, unsigned* failed, int64_t NP, int V, int K, uint64_t seed, double floor, int first, int count,
                             hipStream_t stream);

#ifdef SALNMF_NBDRAW_KERNELS  // salnmf_batch.hip: after salnmf_nbdraw.h
// One workgroup per (pair, draw): nb_draw_kernel's body with the exposure row, the sample's constants and the draw word of the pair.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) nb_presence_draw_kernel(NbPresenceDrawArgs a) {
    const int64_t j = blockIdx.x;
    const int n = a.pair_n[j], s = a.pair_s[j];
    nb_draw_row(a.H0 + (size_t)j * a.K, a.W, a.alpha[n], a.gd[n], a.gc[n], a.out + ((size_t)blockIdx.y * a.NP + j) * a.V, a.failed, a.V, a.K, a.key0,
                a.key1, (uint32_t)n, ((uint32_t)(s + 1) << 16) | (blockIdx.y + a.first), a.floor);
}
#endif  // SALNMF_NBDRAW_KERNELS

#if defined(SALNMF_REFIT_KERNELS) && defined(SALNMF_NB_KERNELS)
template <int KT>
__global__ void __launch_bounds__(BLOCK) nb_presence_kernel(NbPresenceArgs a) {
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
        const double al = a.alpha[n];
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
                const double cur = nb_objective(x, pr, al, V, q);
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
            d4 un[KT];
            nb_update_factors<KT>(x, pr, al, wu, V, q, un, [&](int kt, const d4& ud) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // (in a pad row ud is 0: the quotient there is taken over 1 and dropped, never 0 0 / 0)
                    const double hn = clip_lo(div_path(h[kt][r] * un[kt][r], 16 * kt + 4 * r + q >= K ? 1.0 : ud[r]), kEps);
                    h[kt][r] = (mode == 2 || h[kt][r] == 0.0) ? h[kt][r] : hn;
                }
            });
            ++itl;
        }
    }
}
#endif  // SALNMF_REFIT_KERNELS && SALNMF_NB_KERNELS

}  // namespace salnmf
