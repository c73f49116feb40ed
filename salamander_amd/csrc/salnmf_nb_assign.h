// Sparse per-sample exposures under the negative-binomial likelihood (include/salnmf.h: salnmf_nb_assign_signatures; DESIGN.md
// section 25): the procedure of sections 14 and 14.1 -- phase 0 on the candidate set, backward elimination with a protected set
// that starts as the required one, and the optional re-addition pass -- with section 23's step and divergence.
//
// A problem is a row x against the fixed W with its sample's dispersion alpha (problem p reads alpha[p % N] and the set words of
// row p % N: a resample carries its sample's dispersion and sets).  A SOLVE from a start h is the negative-binomial refit's
// iteration on the entries that are not 0.0:
//   p = h W, a_v = x_v / p_v, b_v = (x_v + alpha) / (p_v + alpha), un_k = sum_v W[k, v] a_v, ud_k = sum_v W[k, v] b_v,
//   h_k <- max((h_k un_k) / ud_k, EPSILON)            (the product first, then one division, as nb_refit_kernel)
// an entry that is 0.0 is left alone (the pad rows k >= K are such entries; there ud is 0 and the divisor is replaced by 1, so that
// 0 0 / 0 is never formed); tests at iteration 0 and at every multiple of conv_test_freq counted from the start of the solve, by
// solve_stop on nb_objective.  The re-addition pass selects by u_k = un_k / ud_k -- ONE division, not the step's quantity, which
// has h inside the numerator -- at the accepted h: the pool member of largest u, lowest index on equal values, goes if u > 1.
//
// nb_assign_kernel is assign_kernel<KT, true> (salnmf_assign.h) statement for statement -- modes 0 to 4, `fresh` and `repass`,
// ballots for the branches and per-column predication inside them, the accepted h parked in the problem's own row of the output
// H, arg-min and arg-max by a lane-local scan in ascending k and two __shfl_xor steps -- around the negative-binomial step and
// objective.  There is one instantiation set, which always takes the sets: null `cand` means all K, null `req` none.
//
// The U phase.  nb_refit_kernel accumulates un and ud side by side on one W operand read.  With this kernel's state on top
// that needs more registers than a lane has, so nb_update_factors accumulates un for every k-tile first, writes b over P^T (P^T
// has no reader after a and b) and then takes one k-tile's ud at a time, handing it to the caller at once.  Every un_k and ud_k
// is the same chain of MFMAs in ascending (vt, r) either way, so the bits are nb_refit_kernel's; the U phase reads W's operands
// twice.  Plain vector stores only; every branch is wave-uniform.
#pragma once
#include "salnmf_assign.h"
#include "salnmf_nb.h"

namespace salnmf {

struct NbAssignArgs {
    const double* __restrict__ X;      // [P][V] compact, clipped
    const double* __restrict__ W;      // [K][V]
    const double* __restrict__ alpha;  // [N]: problem p reads alpha[p % N]
    double* H;                         // [P][K]: the accepted exposures while the kernel runs, the result after it
    double* __restrict__ err;          // [P]
    long long* __restrict__ nit;       // [P]: iterations summed over the solves
    int* __restrict__ conv;            // [P]: every solve stopped on its tolerance
    int* __restrict__ ntrials;         // [P]
    int* __restrict__ active;          // [P][K], or null
    int* __restrict__ round;           // [P][K]: the trial that removed k, -1 if kept; or null
    double* __restrict__ kl;           // [P][K]: f' - f of the trial that tested k, NaN if never tested; or null
    double* __restrict__ dH;           // phase 0 ([P][K], [P], [P], [P]), or all four null
    double* __restrict__ derr;
    int* __restrict__ dnit;
    int* __restrict__ dconv;
    unsigned* next_tile;               // zero at launch
    int64_t P;
    int V, K;
    int min_it, max_it, freq;          // max_it % freq == 0
    double tol, thr;
    const unsigned* __restrict__ cand;  // [N][NW] candidate words of sample n, NW = (KT + 1) / 2; or null: all K
    const unsigned* __restrict__ req;   // [N][NW] required words (a subset of cand); or null: none
    int* __restrict__ rround;           // [P][K]: the trial that re-added k, -1 otherwise; or null
    double* __restrict__ kld;           // [P][K]: f - f' of the re-addition trial of k, NaN if never tried; or null
    int64_t N;                          // rows of alpha / cand / req
    int readd;
};

#if defined(SALNMF_REFIT_KERNELS) && defined(SALNMF_NB_KERNELS)

// un[kt] for every k-tile, then out(kt, ud_kt) for kt = 0 .. KT - 1 with that tile's denominators.  P^T is overwritten by b.
template <int KT, typename Out>
__device__ __forceinline__ void nb_update_factors(const double (&x)[VT][4], d4 (&pr)[VT], double al, const double* wu, int V, int q, d4 (&un)[KT],
                                                  Out&& out) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) un[kt] = (d4){0, 0, 0, 0};
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool in = 16 * vt + 4 * r + q < V;
            const double av = in ? div_path(x[vt][r], pr[vt][r]) : 0.0;
            pr[vt][r] = in ? div_path(x[vt][r] + al, pr[vt][r] + al) : 0.0;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) un[kt] = mfma(wu[16 * kt * WS + 4 * (4 * vt + r)], av, un[kt]);
        }
    }
    // (the second pass reads W's operands anew: without the fence the compiler keeps all 24 KT of the first pass in registers)
    int again = 0;
    asm volatile("" : "+v"(again));
    const double* wd = wu + again;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        d4 ud = (d4){0, 0, 0, 0};
#pragma unroll
        for (int vt = 0; vt < VT; ++vt)
#pragma unroll
            for (int r = 0; r < 4; ++r) ud = mfma(wd[16 * kt * WS + 4 * (4 * vt + r)], pr[vt][r], ud);
        out(kt, ud);
    }
}

template <int KT>
__global__ void __launch_bounds__(BLOCK) nb_assign_kernel(NbAssignArgs a) {
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
        const int64_t sample = row % a.N;
        const double al = a.alpha[sample];
        // the column's state, the same in its four lanes.  A lane column past the end of the list is finished from the start:
        // it recomputes the last problem's first step and touches no memory.
        unsigned act[NW], prot[NW], tried[NW];  // tried: tried for re-addition, or no candidate at all
        d4 h[KT];
        int nc = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int n = K - 32 * w;
            act[w] = n >= 32 ? ~0u : n > 0 ? (1u << n) - 1u : 0u;
            prot[w] = 0u;
            if (a.cand) act[w] &= a.cand[sample * NW + w];
            if (a.req) prot[w] = a.req[sample * NW + w] & act[w];
            tried[w] = ~act[w];
            nc += __popc(act[w]);
        }
        const double h0 = t / (double)nc;  // sum(x) / |C|
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[kt][r] = ((act[kt >> 1] >> ((16 * kt + 4 * r + q) & 31)) & 1u) ? h0 : 0.0;
        int mode = p < a.P ? 0 : 2;  // 0: phase 0, 1: a trial, 2: finished, 3: a re-addition trial, 4: waits for its candidate
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
        if (mode == 0 && a.kld) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * kt + 4 * r + q;
                    if (k < K) a.kld[p * K + k] = __builtin_nan(""), a.rround[p * K + k] = -1;
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
                const double cur = nb_objective(x, pr, al, V, q);
                bool stop = false;
                int cv = 0;
                if (mode != 2 && (fresh || !repass)) {
                    stop = solve_stop(itl, prev, cur, a.min_it, a.max_it, a.tol, cv);
                    prev = cur;
                }
                fresh = false;
                const bool select = mode == 4;  // (asked for this re-pass: P^T is that of the accepted h)
                if (__any(stop)) {
                    const bool dense = stop && mode == 0, trial = stop && mode == 1, add = stop && mode == 3;
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
                    if (a.readd) {
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
                const bool selecting = __any(select);  // (uniform)
                if (selecting) {
                    // the next re-addition candidate: largest un / ud in the pool, lowest index on ties.  The factors overwrite
                    // P^T, so a re-pass always follows and forms it anew (below)
                    d4 u[KT];
                    nb_update_factors<KT>(x, pr, al, wu, V, q, u, [&](int kt, const d4& ud) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) u[kt][r] = div_path(u[kt][r], 16 * kt + 4 * r + q >= K ? 1.0 : ud[r]);
                    });
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
                if (__all(mode == 2)) break;
                if (__any(fresh || mode == 4) || selecting) {
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
