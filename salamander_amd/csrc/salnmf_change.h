// Have the exposure SHARES changed between two samples of one patient?  A parametric-bootstrap p-value per sample pair for a
// nested pair of models (include/salnmf.h: salnmf_exposure_change).
//
// A PAIR is row n of two count matrices with one candidate set C, |C| >= 2 and both integer totals positive; the others are
// untested and never reach the device.  A problem is a pair of rows (x_a, x_b): the pair's own counts (the observed launch) or
// one null draw of it.  Its three SOLVES are those defined at the top of salnmf_assign.h, each on C from a cold start:
//   a       on x_a                  -> f_a (and h_a for an observed problem)
//   b       on x_b                  -> f_b (and h_b)
//   pooled  on x_p = x_a + x_b      -> f_p (and h_0); its start is the row sum of x_p in solve_load_row's order
// bit for bit what assign_kernel<KT, true> returns with candidates = required = C on that row.  Under the null -- the same
// shares, free totals -- sample a's model is c_a P_0 and sample b's c_b P_0, with P_0 = h_0 W, c_a = t_a / (t_a + t_b),
// c_b = t_b / (t_a + t_b) and t the rows' sums: g_a = KL(x_a || c_a P_0), g_b = KL(x_b || c_b P_0), each refit_objective's
// sum term by term on the P^T the pooled solve holds at its stopping test.  The statistic is (g_a - f_a) + (g_b - f_b).
//
// Null draw b of pair n is two model draws of salnmf_gof.h, steps 1-6, from the spectrum h_0 W, one with x_a's total and one
// with x_b's, under the Philox counter (q, 0x43480000 + side, n, b), side 0 for a and 1 for b: the second word carries the
// stream family "CH" -- no other draw's word has these upper 16 bits (salnmf_presence.h lists the four others) -- so a pair's
// draws depend on (seed, n, side, b) and on h_0, and on nothing else.  They lie as [draw][pair][2][V].
//
// change_kernel is presence_kernel's frame (salnmf_presence.h) with three solves in a column instead of two: at the end of
// solve a the column takes x from row b, at the end of solve b it adds row a to the x it holds, and at the end of the pooled
// solve it evaluates the two null divergences from the P^T in its registers against the two rows read again.  Branches are
// taken on ballots, the transitions are predicated per column, and a column's numbers never meet another column's
// (salnmf_refit.h).  A draw problem leaves the statistic and its three iteration counts; an observed problem also its three
// exposure rows, five divergences and three convergence flags.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace salnmf {

constexpr uint32_t CHANGE_STREAM = 0x43480000u;  // "CH" << 16: the second counter word of a block is this plus the side (0: a, 1: b)

struct ChangeArgs {
    const double* __restrict__ Xa;      // row r of side a is Xa + r * stride, of side b Xb + r * stride.  by_sample: r = pair_n[p]
    const double* __restrict__ Xb;      // (the two clipped count matrices); otherwise r = p (the interleaved chunk of draws)
    const double* __restrict__ W;       // [K][V]
    const int* __restrict__ pair_n;     // [NP] the row of pair j in the count matrices; problem p belongs to pair p % NP
    const unsigned* __restrict__ cand;  // [N][NW] candidate words of row n, NW = (KT + 1) / 2; or null: all K
    double* __restrict__ stat;          // [P] (g_a - f_a) + (g_b - f_b)
    int* __restrict__ nit;              // [P][3] iterations of the solves a, b, pooled
    double* __restrict__ f;             // [P][5] f_a, f_b, f_p, g_a, g_b;      observed launch, else null
    int* __restrict__ conv;             // [P][3]                                with f
    double* __restrict__ Ha;            // [P][K]                                with f
    double* __restrict__ Hb;            // [P][K]                                with f
    double* __restrict__ H0;            // [P][K] the pooled solve's             with f
    unsigned* next_tile;                // zero at launch
    int64_t P, NP, stride;
    int V, K, by_sample;
    int min_it, max_it, freq;  // max_it % freq == 0
    double tol;
};

struct ChangeDrawArgs {
    const double* __restrict__ H0;   // [NP][K] the pooled fit's exposures of every pair, where the observed launch left them
    const double* __restrict__ W;    // [K][V]
    const double* __restrict__ Xa;   // [N][V] the clipped counts: a row's trial count is sum_v (uint32) X[n, v]
    const double* __restrict__ Xb;   // [N][V]
    const int* __restrict__ pair_n;  // [NP]
    double* __restrict__ out;        // [draws][NP][2][V]
    int64_t NP;
    int V, K;
    uint32_t key0, key1;
    double floor;
    uint32_t first;  // slot 0 of `out` holds draw `first`
};

// salnmf_batch.hip (the translation unit of model_draw_kernel): draws first .. first + count - 1 of every pair as out[count][NP][2][V]
void change_launch_draw(const double* H0, const double* W, const double* Xa, const double* Xb, const int* pair_n, double* out, int64_t NP, int V,
                        int K, uint64_t seed, double floor, int first, int count, hipStream_t stream);

#ifdef SALNMF_GOF_KERNELS  // salnmf_batch.hip: after salnmf_gof.h
// One workgroup per (pair, side, draw): blockIdx.x = 2 pair + side, blockIdx.y = draw - a.first.  model_draw_kernel's body with the
// pooled exposure row, the side's own total and the stream word of the side.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) change_draw_kernel(ChangeDrawArgs a) {
    const int64_t j = blockIdx.x >> 1;
    const uint32_t side = blockIdx.x & 1u;
    const int n = a.pair_n[j];
    model_draw_row(a.H0 + (size_t)j * a.K, a.W, nullptr, (side ? a.Xb : a.Xa) + (size_t)n * a.V,
                   a.out + (((size_t)blockIdx.y * a.NP + j) * 2 + side) * a.V, a.V, a.K, a.key0, a.key1, CHANGE_STREAM + side, (uint32_t)n,
                   blockIdx.y + a.first, a.floor);
}
#endif  // SALNMF_GOF_KERNELS

#ifdef SALNMF_REFIT_KERNELS  // salnmf_refit.hip: after salnmf_assign.h

// KL(xs || c P) of one column from the lane's 24 entries of P^T, the row read again: refit_objective's term per entry with
// p_v = c P_v (one rounded product), the lane's entries in (vt, r) order, then the four q groups by rows_sum.
__device__ __forceinline__ double change_null_divergence(const double* xs, const d4 (&pr)[VT], double c, int V, int q) {
    double acc = 0.0;
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = 16 * vt + 4 * r + q;
            if (v < V) {
                const double xv = xs[v], pv = c * pr[vt][r];
                const double xe = (xv == 0.0) ? kEps : xv, pe = (xv == 0.0) ? kEps : pv;
                const double l = (log_operand_ok(xe) && log_operand_ok(pe)) ? log_ratio(xe, pe) : log(xe / pe);
                acc += xe * l - xv + pv;
            }
        }
        asm volatile("" : "+v"(acc));  // as refit_objective: four logarithms side by side
    }
    return rows_sum(acc);
}

template <int KT>
__global__ void __launch_bounds__(BLOCK) change_kernel(ChangeArgs a) {
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
        const int n = a.pair_n[row % a.NP];
        // a lane column past the end of the list is finished from the start: it recomputes the last problem's first step, reads
        // that problem's rows at the transitions of the others and stores nothing
        const int64_t off = (a.by_sample ? (int64_t)n : row) * a.stride;  // of the problem's row in Xa and in Xb
        double x[VT][4];
        const double ta = solve_load_row(a.Xa + off, V, q, x);
        unsigned act[NW];
        const int nc = solve_candidate_words<NW>(K, a.cand, (int64_t)n * NW, act);
        d4 h[KT];
        auto start = [&](double t) {
            const double h0 = t / (double)nc;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) h[kt][r] = ((act[kt >> 1] >> ((16 * kt + 4 * r + q) & 31)) & 1u) ? h0 : 0.0;
        };
        start(ta);
        int mode = p < a.P ? 0 : 3;  // 0: the solve on x_a, 1: on x_b, 2: on x_a + x_b, 3: finished
        bool fresh = false;          // the solve has just started: its iteration-0 test is due
        int itl = 0;
        double prev = 0.0, tb = 0.0, fa = 0.0, fb = 0.0;
        auto latch = [&](double* H, int which, double cur, int cv) {  // (the caller's predicate holds)
            if (H) solve_store_column<KT>(H + p * K, h, K, q);
            if (q == 0) {
                a.nit[3 * p + which] = itl;
                if (a.f) a.f[5 * p + which] = cur, a.conv[3 * p + which] = cv;
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
                if (mode != 3 && (fresh || !repass)) {
                    stop = solve_stop(itl, prev, cur, a.min_it, a.max_it, a.tol, cv);
                    prev = cur;
                }
                fresh = false;
                if (__any(stop)) {
                    const bool end_p = stop && mode == 2, end_b = stop && mode == 1, end_a = stop && mode == 0;
                    if (__any(end_p)) {  // (uniform: every column evaluates, the ending ones keep it)
                        const double tp = ta + tb;
                        const double ga = change_null_divergence(a.Xa + off, pr, ta / tp, V, q);
                        const double gb = change_null_divergence(a.Xb + off, pr, tb / tp, V, q);
                        if (end_p) {
                            latch(a.H0, 2, cur, cv);
                            if (q == 0) {
                                a.stat[p] = (ga - fa) + (gb - fb);
                                if (a.f) a.f[5 * p + 3] = ga, a.f[5 * p + 4] = gb;
                            }
                            mode = 3;
                        }
                    }
                    if (__any(end_a || end_b)) {  // (uniform)
                        if (end_a) latch(a.Ha, 0, cur, cv), fa = cur;
                        if (end_b) latch(a.Hb, 1, cur, cv), fb = cur;
                        // the next solve's row: row b after solve a, the held row b plus row a after solve b; its sum in
                        // solve_load_row's order.  The other columns keep their x.
                        const double* src = (end_a ? a.Xb : a.Xa) + off;
                        double t = 0.0;
#pragma unroll
                        for (int vt = 0; vt < VT; ++vt)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int v = 16 * vt + 4 * r + q;
                                const double other = v < V ? src[v] : 0.0;
                                const double next = end_a ? other : x[vt][r] + other;
                                x[vt][r] = (end_a || end_b) ? next : x[vt][r];
                                t += x[vt][r];
                            }
                        t = rows_sum(t);
                        if (end_a) tb = t;
                        if (end_a || end_b) {
                            start(t);
                            mode += 1, itl = 0, fresh = true;
                        }
                    }
                }
                if (__all(mode == 3)) break;
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
                    h[kt][r] = (mode == 3 || h[kt][r] == 0.0) ? h[kt][r] : hn;
                }
            ++itl;
        }
    }
}
#endif  // SALNMF_REFIT_KERNELS

}  // namespace salnmf
