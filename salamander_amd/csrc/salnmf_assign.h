// Sparse per-sample exposures by backward elimination inside the refit's step loop (include/salnmf.h:
// salnmf_assign_signatures).
//
// A problem is a row x against the fixed W, as in salnmf_refit.h.  A SOLVE from a start h with an active set A is the refit's
// iteration on the active entries: same step, same objective, same stop rule, iterations counted from 0 at the start of the
// solve; inactive entries are exactly 0.0 and stay 0.0 (a step leaves an entry that is 0.0 alone, which also covers the pad
// rows k >= K; an active entry is >= EPSILON after a step and sum(x) / K > 0 before the first, so "0.0" and "inactive" are the
// same thing).  Phase 0 solves with all K from h_k = sum(x) / K: the refit itself, bit for bit.  Then rounds: the candidate c is
// the active, not yet protected signature of smallest h (lowest index on equal values); the trial copies h, sets entry c to
// 0.0 and solves; if f' - f <= max_kl_increase (false for a NaN) the trial's h, f and A \ {c} are accepted, otherwise c is
// protected for good and h, f stay.  The procedure ends when there is no candidate or one signature is left.
//
// assign_kernel is refit_kernel with a state machine per lane column, on the same solve_* pieces (salnmf_refit.h).  max_iterations is a multiple of conv_test_freq, so
// every solve ends at a test and the next one starts there: the tests of all 16 columns fall on the same iterations of the
// wave's loop whatever each column is doing.  At a test where some column's solve ends, those columns take their decision,
// write their next start into h, and the loop body runs again from the P^T product without stepping: that pass is the new
// solves' iteration-0 test (the other columns recompute the bits they had and skip it).  The accepted h of a problem lives in
// its own row of the output H -- stored by the lane that owns the entry and, after a rejected trial, loaded back by the same
// lane -- so the loop carries one h, not two.  The sets are bit masks held alike by the four lanes of a column.  Branches
// are taken on ballots, the transitions inside them are predicated per column; a column's numbers never meet another
// column's (salnmf_refit.h), so a problem's result depends on nothing but its row and W.
//
// assign_kernel<KT, true> adds candidate sets, required signatures and the re-addition pass; the
// <KT, false> instantiations are the kernel above, statement for statement.  The act / prot words start from two optional
// per-sample arrays (problem p reads row p % N: a resample shares its sample's sets) and the start value divides by the
// population count of the candidate words.  A third set, `tried`, starts as the complement of the candidates, so the pool of
// the re-addition pass is ~act & ~tried.  Two more modes: 4, the column waits for its next re-addition candidate, and 3, a
// re-addition trial.  A column whose backward rounds are over (or whose re-addition trial has been decided) goes to mode 4
// and asks for a re-pass; there P^T is that of the accepted h (reloaded after a rejection), the update factors U are
// computed from it as a step computes them, and the column takes the pool member of largest U, lowest index on equal values
// -- lane-local in ascending k, then two __shfl_xor steps, as the arg-min.  If U > 1 its entry is set to sum(x) / |C| and
// the solve starts (mode 3, one more re-pass for its iteration-0 test), otherwise the column is finished.
#pragma once
#include "salnmf_refit.h"

namespace salnmf {

struct AssignArgs {
    const double* __restrict__ X;  // [P][V] compact, clipped
    const double* __restrict__ W;  // [K][V]
    double* H;                     // [P][K]: the accepted exposures while the kernel runs, the result after it
    double* __restrict__ err;      // [P]
    long long* __restrict__ nit;   // [P]: iterations summed over the solves
    int* __restrict__ conv;        // [P]: every solve stopped on its tolerance
    int* __restrict__ ntrials;     // [P]
    int* __restrict__ active;      // [P][K], or null
    int* __restrict__ round;       // [P][K]: the round that removed k, -1 if kept; or null
    double* __restrict__ kl;       // [P][K]: f' - f of the trial that tested k, NaN if never tested; or null
    double* __restrict__ dH;       // phase 0 ([P][K], [P], [P], [P]), or all four null
    double* __restrict__ derr;
    int* __restrict__ dnit;
    int* __restrict__ dconv;
    unsigned* next_tile;           // zero at launch
    int64_t P;
    int V, K;
    int min_it, max_it, freq;      // max_it % freq == 0
    double tol, thr;
    // assign_kernel<KT, true> alone reads what follows
    const unsigned* __restrict__ cand;  // [N][NW] candidate words of sample n, NW = (KT + 1) / 2; or null: all K
    const unsigned* __restrict__ req;   // [N][NW] required words (a subset of cand); or null: none
    int* __restrict__ rround;           // [P][K]: the trial that re-added k, -1 otherwise; or null
    double* __restrict__ kld;           // [P][K]: f - f' of the re-addition trial of k, NaN if never tried; or null
    int64_t N;                          // rows of cand / req: problem p reads row p % N
    int readd;
};

struct AssignSelectArgs {
    const double* __restrict__ H;  // [R][NK]
    double* __restrict__ freq;     // [NK]
    int64_t NK;
    int R;
};

// salnmf_refit.hip (the translation unit of assign_selection_kernel): freq [NK] from the resamples' exposures H [R][NK]
void assign_launch_selection(const double* H, double* freq, int64_t NK, int R, hipStream_t stream);

#ifdef SALNMF_REFIT_KERNELS

template <int KT, bool EX>
__global__ void __launch_bounds__(BLOCK) assign_kernel(AssignArgs a) {
    constexpr int KP = 16 * KT;
    constexpr int NW = (KT + 1) / 2;  // 32-bit words of a signature set
    constexpr int NONE = 0x7fffffff;
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
        double* hrow = a.H + row * K;
        double x[VT][4];
        const double t = solve_load_row(a.X + row * V, V, q, x);
        // the column's state, the same in its four lanes.  A lane column past the end of the list is finished from the start:
        // it recomputes the last problem's first step and touches no memory.
        unsigned act[NW], prot[NW];
        [[maybe_unused]] unsigned tried[NW];  // EX: tried for re-addition, or no candidate at all
        [[maybe_unused]] double h0 = 0.0;     // EX: sum(x) / |C|
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int n = K - 32 * w;
            act[w] = n >= 32 ? ~0u : n > 0 ? (1u << n) - 1u : 0u;
            prot[w] = 0u;
        }
        d4 h[KT];
        if constexpr (EX) {
            const int64_t mrow = (row % a.N) * NW;
            int nc = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                if (a.cand) act[w] &= a.cand[mrow + w];
                if (a.req) prot[w] = a.req[mrow + w] & act[w];
                tried[w] = ~act[w];
                nc += __popc(act[w]);
            }
            h0 = t / (double)nc;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) h[kt][r] = ((act[kt >> 1] >> ((16 * kt + 4 * r + q) & 31)) & 1u) ? h0 : 0.0;
        } else {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) h[kt][r] = (16 * kt + 4 * r + q < K) ? t / (double)K : 0.0;
        }
        int mode = p < a.P ? 0 : 2;  // 0: phase 0, 1: a trial, 2: finished; EX: 3: a re-addition trial, 4: waits for its candidate
        bool fresh = false;          // the solve has just started: its iteration-0 test is due
        int itl = 0, cand = 0, ntr = 0, conv = 1;
        long long nsum = 0;
        double prev = 0.0, f = 0.0;
        if (mode == 0 && a.kl) {  // (the lane that owns entry k writes it here and later: program order)
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * kt + 4 * r + q;
                    if (k < K) a.kl[p * K + k] = __builtin_nan(""), a.round[p * K + k] = -1;
                }
        }
        if constexpr (EX) {
            if (mode == 0 && a.kld) {
#pragma unroll
                for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int k = 16 * kt + 4 * r + q;
                        if (k < K) a.kld[p * K + k] = __builtin_nan(""), a.rround[p * K + k] = -1;
                    }
            }
        }
        // the column is through: its sets and sums go out (predicated)
        auto finish = [&](bool who) {
            if (who) {
                mode = 2;
                if (a.active) {
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int k = 16 * kt + 4 * r + q;
                            if (k < K) a.active[p * K + k] = (int)((act[kt >> 1] >> (k & 31)) & 1u);
                        }
                }
                if (q == 0) a.err[p] = f, a.nit[p] = nsum, a.conv[p] = conv, a.ntrials[p] = ntr;
            }
        };

        int until_test = 0;   // steps until the next multiple of conv_test_freq (uniform)
        bool repass = false;  // this pass of the body follows a transition without a step (uniform)
        for (;;) {
            d4 pr[VT];
#pragma unroll
            for (int vt = 0; vt < VT; ++vt) pr[vt] = (d4){0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4 * KT; ++s) {
                const double b = h[s >> 2][s & 3];
#pragma unroll
                for (int vt = 0; vt < VT; ++vt) pr[vt] = mfma(wp[4 * s * WS + 16 * vt], b, pr[vt]);
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
                [[maybe_unused]] const bool select = EX && mode == 4;  // (asked for this re-pass: P^T is that of the accepted h)
                if (__any(stop)) {
                    const bool dense = stop && mode == 0, trial = stop && mode == 1, add = EX && stop && mode == 3;
                    const double delta = add ? f - cur : cur - f;
                    const bool accept = dense || (trial && delta <= a.thr) || (add && delta > a.thr), reject = (trial || add) && !accept;
                    const bool owner = q == (cand & 3);
                    if (stop) nsum += itl, conv &= cv;
                    if (dense && a.dH) {
                        solve_store_column<KT>(a.dH + p * K, h, K, q);
                        if (q == 0) a.derr[p] = cur, a.dnit[p] = itl, a.dconv[p] = cv;
                    }
                    if (trial && owner && a.kl) a.kl[p * K + cand] = delta;
                    if (trial && accept) {
                        if (owner && a.round) a.round[p * K + cand] = ntr;
#pragma unroll
                        for (int w = 0; w < NW; ++w) act[w] &= ~((cand >> 5) == w ? 1u << (cand & 31) : 0u);
                    }
                    if (reject) {
#pragma unroll
                        for (int w = 0; w < NW; ++w) prot[w] |= (cand >> 5) == w ? 1u << (cand & 31) : 0u;
                    }
                    if constexpr (EX) {
                        if (add && owner && a.kld) a.kld[p * K + cand] = delta;
                        if (add && accept && owner && a.rround) a.rround[p * K + cand] = ntr;
                        if (add) {
#pragma unroll
                            for (int w = 0; w < NW; ++w) {
                                const unsigned bit = (cand >> 5) == w ? 1u << (cand & 31) : 0u;
                                tried[w] |= bit;
                                act[w] |= accept ? bit : 0u;
                            }
                        }
                    }
                    if (trial || add) ++ntr;
                    if (accept) f = cur;
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int k = 16 * kt + 4 * r + q;
                            if (accept && k < K) hrow[k] = h[kt][r];
                            if (reject) h[kt][r] = k < K ? hrow[k] : 0.0;
                        }
                    // the next candidate: smallest accepted h among the active, unprotected entries, lowest index on ties --
                    // the lane's own entries in ascending k, then across the four q groups
                    unsigned el[NW];
                    int left = 0;
#pragma unroll
                    for (int w = 0; w < NW; ++w) el[w] = (act[w] & ~prot[w]) >> q, left += __popc(act[w]);
                    double bv = __builtin_inf();
                    int bi = NONE;
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const bool ok = (el[kt >> 1] >> (16 * (kt & 1) + 4 * r)) & 1u;
                            if (ok && h[kt][r] < bv) bv = h[kt][r], bi = 16 * kt + 4 * r + q;
                        }
#pragma unroll
                    for (int m = 16; m <= 32; m <<= 1) {
                        const double ov = __shfl_xor(bv, m);
                        const int oi = __shfl_xor(bi, m);
                        if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
                    }
                    const bool more = stop && !add && bi != NONE && left > 1;
                    if (EX && a.readd) {
                        if (stop && !more) mode = 4;
                    } else {
                        finish(stop && !more);
                    }
                    if (more) {
                        cand = bi, mode = 1, itl = 0, fresh = true;
#pragma unroll
                        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (16 * kt + 4 * r + q == bi) h[kt][r] = 0.0;
                    }
                }
                if constexpr (EX) {
                    if (__any(select)) {
                        // the next re-addition candidate: largest update factor in the pool, lowest index on ties
                        d4 u[KT];
                        solve_update_factors<KT>(x, pr, wu, V, q, u);
                        unsigned el[NW];
#pragma unroll
                        for (int w = 0; w < NW; ++w) el[w] = (~act[w] & ~tried[w]) >> q;
                        double bv = -__builtin_inf();
                        int bi = NONE;
#pragma unroll
                        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const bool ok = (el[kt >> 1] >> (16 * (kt & 1) + 4 * r)) & 1u;
                                if (ok && u[kt][r] > bv) bv = u[kt][r], bi = 16 * kt + 4 * r + q;
                            }
#pragma unroll
                        for (int m = 16; m <= 32; m <<= 1) {
                            const double ov = __shfl_xor(bv, m);
                            const int oi = __shfl_xor(bi, m);
                            if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
                        }
                        const bool go = select && bi != NONE && bv > 1.0;
                        finish(select && !go);
                        if (go) {
                            cand = bi, mode = 3, itl = 0, fresh = true;
#pragma unroll
                            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    if (16 * kt + 4 * r + q == bi) h[kt][r] = h0;
                        }
                    }
                }
                if (__all(mode == 2)) break;
                if (__any(fresh || (EX && mode == 4))) {
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

#ifdef SALNMF_ASSIGN_SELECT_KERNEL  // salnmf_refit.hip alone: an ordinary kernel, defined once in the library (assign_launch_selection)

// selection_frequency[n][k] = (resamples whose exposure of k in n is > 0) / R, counted in integers
__global__ void __launch_bounds__(256) assign_selection_kernel(AssignSelectArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.NK) return;
    int c = 0;
    for (int r = 0; r < a.R; ++r) c += a.H[(size_t)r * a.NK + i] > 0.0 ? 1 : 0;
    a.freq[i] = (double)c / (double)a.R;
}
#endif  // SALNMF_ASSIGN_SELECT_KERNEL

}  // namespace salnmf
