// The profile likelihood of one exposure, and the interval it gives (include/salnmf.h: salnmf_profile_likelihood,
// salnmf_exposure_intervals).
//
// A PAIR is that of salnmf_presence.h: a sample n with candidate set C and a signature s in C, |C| >= 2.  The FROZEN SOLVE of a
// pair at a value c >= 0 starts from h_s = c, h_k = sum(x) / (|C| - 1) on C \ {s} and exactly 0.0 off C; every step applies the
// refit's update factors with the kEps clip to the members of C \ {s} and leaves h_s alone; the objective is the sample's KL
// divergence at the whole h, and the stop rule the refit's.  Its result is f(c).  At c = 0.0 the frozen entry adds exact zeros
// to every product and the solve is bit for bit presence_kernel's null solve.
//
// A PROBLEM is a column of trials, one frozen solve after another from cold starts:
//   grid mode    (pair, one run of the caller's values): trial i solves at values[p][i], i < count[p];
//   search mode  (pair, end): the trial values come from the search rule below, fed by g(c) = f(c) - f1 with the pair's
//                alternative fit f1, threshold delta, J = n_bisections and E = max_expansions.  With hh the pair's estimate:
//     lower end (listed only where g(0) <= delta is false): lo = 0.0, hi = hh; J times m = 0.5 (lo + hi), g(m) > delta ? lo = m
//                : hi = m.  While lo is still 0.0 after them -- the root lies below hh / 2^J -- the halving goes on, at most E
//                more times, and stops at the first trial outside: a searched lower end is 0.0 only if none of the J + E
//                trials lay outside.  The end is lo.
//     upper end: d = hh > 1.0 ? hh : 1.0, lo = hh; expansion trial e = 0, 1, .. is c = hh + d 2^e (d doubled e times, exact);
//                g(c) > delta ? hi = c, stop expanding : lo = c; after E trials without a bracket the end is +inf
//                (bracketed = 0); otherwise J times m = 0.5 (lo + hi), g(m) > delta ? hi = m : lo = m; the end is hi.
//     A comparison with a NaN is false.  Both ends are the outer ones of their last bracket.
//
// profile_kernel is presence_kernel's tile loop and tile tickets (on the solve_* pieces of salnmf_refit.h where they cost
// it no register) with its two-state mode made a per-column trial machine: a
// column whose solve ends at a test stores the trial, takes its next value, resets its start and runs the loop body again from
// the P^T product without stepping -- the next solve's iteration-0 test -- exactly as the null solve follows the alternative
// there.  The frozen signature is one bit beside act[]; the step keeps an entry that is finished, 0.0 or frozen.  x is loaded
// once per problem, branches are taken on ballots, transitions are predicated per column, a column's numbers never meet another
// column's, and every store is a plain vector store.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace salnmf {

constexpr int PROFILE_MAX_VALUES = 4096;     // values per pair of a grid call
constexpr int PROFILE_RUN = 8;               // values of one grid problem: a pair's values are split into runs of this length
constexpr int PROFILE_MAX_BISECTIONS = 64;   // more halve nothing in fp64
constexpr int PROFILE_MAX_EXPANSIONS = 1000;  // d 2^e stays finite up to here for every d a count matrix can give

struct ProfileArgs {
    const double* __restrict__ X;       // [N][V], problem p reads row prob_n[p]
    const double* __restrict__ W;       // [K][V]
    const int* __restrict__ prob_n;     // [P] the sample of problem p
    const int* __restrict__ prob_s;     // [P] its frozen signature
    const unsigned* __restrict__ cand;  // [N][NW] candidate words of sample n, NW = (KT + 1) / 2; or null: all K
    const double* __restrict__ values;  // grid mode: [P][T] the trial values; null in search mode
    const int* __restrict__ count;      // grid mode: [P] trials of problem p, in [1, T]
    const int* __restrict__ end;        // search mode: [P] 0 the lower end, 1 the upper
    const double* __restrict__ hhat;    // search mode: [P] the pair's estimate hh
    const double* __restrict__ f1;      // search mode: [P] the pair's alternative fit
    double* __restrict__ trial_c;       // search mode: [P][T] the trial values in trial order
    double* __restrict__ trial_f;       // [P][T] f of every trial
    int* __restrict__ trial_nit;        // [P][T]
    int* __restrict__ trial_conv;       // [P][T]
    double* __restrict__ trial_H;       // [P][T][K] the trial's exposures, or null
    double* __restrict__ lo;            // search mode: [P] the last bracket
    double* __restrict__ hi;            // search mode: [P]
    int* __restrict__ n_trials;         // search mode: [P]
    int* __restrict__ bracketed;        // search mode: [P]
    unsigned* next_tile;                // zero at launch
    int64_t P;
    int V, K, T;  // T: trials a problem has room for (search mode: E + J)
    int n_bisections, max_expansions;
    double delta;
    int min_it, max_it, freq;  // max_it % freq == 0
    double tol;
};

#ifdef SALNMF_REFIT_KERNELS  // salnmf_refit.hip: after salnmf_assign.h
template <int KT>
__global__ void __launch_bounds__(BLOCK) profile_kernel(ProfileArgs a) {
    constexpr int KP = 16 * KT;
    constexpr int NW = (KT + 1) / 2;  // 32-bit words of a signature set
    __shared__ double Wl[KP * WS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c16 = lane & 15, q = lane >> 4;
    const int V = a.V, K = a.K;
    for (int i = tid; i < KP * WS; i += BLOCK) {
        const int k = i / WS, v = i - k * WS;
        Wl[i] = (k < K && v < V) ? a.W[k * V + v] : 0.0;
    }
    __syncthreads();
    const int64_t ntiles = (a.P + 15) / 16;
    const double* wp = Wl + q * WS + c16;
    const double* wu = Wl + c16 * WS + q;
    const bool search = a.values == nullptr;

    for (;;) {
        unsigned ticket = 0;
        if (lane == 0) ticket = atomicAdd(a.next_tile, 1u);
        const int64_t tile = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)ticket);
        if (tile >= ntiles) break;
        const int64_t p = tile * 16 + c16;
        const int64_t row = p < a.P ? p : a.P - 1;
        const int n = a.prob_n[row], s = a.prob_s[row];
        const double* xs = a.X + (int64_t)n * V;
        double x[VT][4];
        double t = 0.0;
#pragma unroll
        for (int vt = 0; vt < VT; ++vt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = 16 * vt + 4 * r + q;
                x[vt][r] = v < V ? xs[v] : 0.0;
                t += x[vt][r];
            }
        t = rows_sum(t);
        // the column's set C and, beside it, the one bit of its frozen signature (the same in its four lanes).  A lane column
        // past the end of the list is finished from the start: it recomputes the last problem's first step and touches no memory.
        unsigned act[NW], frz[NW];
        int nc = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int m = K - 32 * w;
            act[w] = m >= 32 ? ~0u : m > 0 ? (1u << m) - 1u : 0u;
            if (a.cand) act[w] &= a.cand[(int64_t)n * NW + w];
            nc += __popc(act[w]);
            frz[w] = (s >> 5) == w ? 1u << (s & 31) : 0u;
        }
        const double h0 = t / (double)(nc - 1);
        d4 h[KT];
        auto start = [&](double c) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * kt + 4 * r + q;
                    const double free_start = ((act[kt >> 1] >> (k & 31)) & 1u) ? h0 : 0.0;
                    h[kt][r] = ((frz[kt >> 1] >> (k & 31)) & 1u) ? c : free_start;
                }
        };
        // the trial machine's state: the bracket, the trial value, the expansion step, and three counters
        const bool upper = search && a.end[row] != 0;
        const double hh = search ? a.hhat[row] : 0.0, f1 = search ? a.f1[row] : 0.0;
        const int todo = search ? 0 : a.count[row];
        double lo = upper ? hh : 0.0, hi = hh, step = hh > 1.0 ? hh : 1.0;
        bool expanding = upper;
        int ti = 0, ne = 0, nb = 0, br = 1;
        double c = search ? (upper ? hh + step : 0.5 * (lo + hi)) : a.values[row * a.T];
        start(c);
        bool done = !(p < a.P);
        bool fresh = false;  // the solve has just started: its iteration-0 test is due
        int itl = 0;
        double prev = 0.0;

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
                if (!done && (fresh || !repass)) {
                    stop = solve_stop(itl, prev, cur, a.min_it, a.max_it, a.tol, cv);
                    prev = cur;
                }
                fresh = false;
                if (__any(stop)) {
                    if (stop) {
                        // the trial's results (ti < T: the host's counts in grid mode; in search mode ne <= E, nb <= J at an upper
                        // and nb <= J + E at a lower end, which does not expand)
                        const int64_t o = p * a.T + ti;
                        if (a.trial_H) solve_store_column<KT>(a.trial_H + o * K, h, K, q);
                        if (q == 0) {
                            a.trial_f[o] = cur, a.trial_nit[o] = itl, a.trial_conv[o] = cv;
                            if (search) a.trial_c[o] = c;
                        }
                        ++ti;
                        if (search) {
                            const bool outside = cur - f1 > a.delta;  // (false for a NaN)
                            if (expanding) {
                                ++ne;
                                if (outside) hi = c, expanding = false;
                                else lo = c, step = step + step;
                                if (expanding && ne == a.max_expansions) done = true, br = 0;
                                c = hh + step;
                            } else {
                                ++nb;
                                if (outside == upper) hi = c;
                                else lo = c;
                            }
                            if (!expanding) {
                                // (a lower end whose bracket still starts at 0.0 goes on halving, at most E more times)
                                if (nb >= a.n_bisections && (upper || lo > 0.0 || nb == a.n_bisections + a.max_expansions)) done = true;
                                c = 0.5 * (lo + hi);
                            }
                            if (done && q == 0) a.lo[p] = lo, a.hi[p] = hi, a.n_trials[p] = ti, a.bracketed[p] = br;
                        } else {
                            if (ti == todo) done = true;
                            else c = a.values[p * a.T + ti];
                        }
                        if (!done) {
                            start(c);
                            itl = 0, fresh = true;
                        }
                    }
                }
                if (__all(done)) break;
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
                    const int k = 16 * kt + 4 * r + q;
                    const double hn = clip_lo(h[kt][r] * u[kt][r], kEps);
                    const bool frozen = (frz[kt >> 1] >> (k & 31)) & 1u;
                    h[kt][r] = (done || h[kt][r] == 0.0 || frozen) ? h[kt][r] : hn;
                }
            ++itl;
        }
    }
}
#endif  // SALNMF_REFIT_KERNELS

}  // namespace salnmf
