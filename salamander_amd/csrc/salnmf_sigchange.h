// WHICH signature's share has changed between two samples of one patient?  A parametric-bootstrap p-value per (sample pair,
// tested signature) for a nested pair of models (include/salnmf.h: salnmf_signature_change).
//
// A PROBLEM is a pair of rows (x_a, x_b) -- row n of two count matrices, or one null draw of it -- with the pair's candidate
// set C, |C| >= 2, a tested signature s in C and both integer totals positive; the others are untested and never reach the
// device.  t_a, t_b are the clipped rows' sums in solve_load_row's order, c_a = t_a / (t_a + t_b), c_b = t_b / (t_a + t_b).  The
// share of s in a sample is h_s / t.  Its three SOLVES, each on C from the cold start h_k = t_side / |C|:
//   a      on x_a                            -> f_a (and h_a for an observed problem)
//   b      on x_b                            -> f_b (and h_b)
//          bit for bit what assign_kernel<KT, true> returns with candidates = required = C on that row;
//   tied   on x_a and x_b side by side under h_as / t_a = h_bs / t_b: every entry but s takes its own column's update factor,
//          entry s takes F = c_a u_as + c_b u_bs in BOTH samples (the EM update of the common share: d/d pi of KL_a + KL_b with
//          rows of W of sum one), evaluated as tied_factor below has it; the EPSILON clip is per sample, so the tie holds
//          except at the floor; the objective is f_a0 + f_b0 (one rounded sum), tested by solve_stop at iteration 0 and at every
//          multiple of conv_test_freq; both samples stop together           -> f_a0, f_b0 (and h_a0, h_b0)
// statistic = (f_a0 - f_a) + (f_b0 - f_b), half the likelihood-ratio statistic with one constrained parameter.  Every sum above
// is of two operands and no product is fused into one, so exchanging the samples exchanges the sides' results and leaves the
// statistic's bits; and where both samples have the same update factor of s the tied step is the free step.
//
// Null draw b of problem (n, s) is two model draws of salnmf_gof.h, steps 1-6: side a from the spectrum h_a0 W with x_a's total,
// side b from h_b0 W with x_b's, under the Philox counter (q, 0x53430000 + 2 s + side, n, b).  The second word carries the stream
// family "SC"; the words of the other draws are 0 (the resampler), 0x53504C54 (the split), 0x474F4644 (goodness of fit),
// 0x5053.... (presence), 0x5057.... (power) and 0x4348.... (the change of all shares): no two families share their upper 16 bits,
// so a problem's draws depend on (seed, n, s, side, b) and on the tied exposures, and on nothing else.  They lie as
// [draw][problem][2][V].
//
// sigchange_kernel is change_kernel's frame (salnmf_change.h) with a problem in TWO adjacent lane columns: column 2 j of a tile
// is side a of its problem j, column 2 j + 1 side b, so a tile of 16 columns is 8 problems and the column list has an even
// length.  A column's mode: 0 the free solve of its own row, 1 that solve latched and the column waiting for its partner, 2 the
// tied solve, 3 finished.  A problem passes to 2 at the first objective test at which both columns are at 1 or beyond 0; both
// then make the cold start.  The partner is lane ^ 1, which holds the same (kt, r, q) of the other sample: the update factors,
// the objective, the mode and the totals cross by a DPP quad_perm:[1,0,3,2] move of the two 32-bit halves, at wave-uniform
// points with every lane active; no LDS but W's.  Branches are taken on ballots, the transitions are predicated per column, and
// a problem's numbers never meet another problem's.  A draw problem leaves the statistic and its three iteration counts; an
// observed problem also its four exposure rows, four divergences and three convergence flags.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace salnmf {

constexpr uint32_t SIGCHANGE_STREAM = 0x53430000u;  // "SC" << 16: the second counter word of a block is this plus 2 s + side (0: a, 1: b)

struct SigChangeArgs {
    const double* __restrict__ Xa;      // row r of side a is Xa + r * stride, of side b Xb + r * stride.  by_sample: r = pair_n[p % NP]
    const double* __restrict__ Xb;      // (the two clipped count matrices); otherwise r = p (the interleaved chunk of draws)
    const double* __restrict__ W;       // [K][V]
    const int* __restrict__ pair_n;     // [NP] the row of listed problem j in the count matrices; problem p belongs to entry p % NP
    const int* __restrict__ pair_s;     // [NP] its tested signature
    const unsigned* __restrict__ cand;  // [N][NW] candidate words of row n, NW = (KT + 1) / 2; or null: all K
    double* __restrict__ stat;          // [P] (f_a0 - f_a) + (f_b0 - f_b)
    int* __restrict__ nit;              // [P][3] iterations of the solves a, b, tied
    double* __restrict__ f;             // [P][4] f_a, f_b, f_a0, f_b0;          observed launch, else null
    int* __restrict__ conv;             // [P][3]                                with f
    double* __restrict__ Ha;            // [P][K]                                with f
    double* __restrict__ Hb;            // [P][K]                                with f
    double* __restrict__ Ha0;           // [P][K] the tied solve's, side a       with f
    double* __restrict__ Hb0;           // [P][K]                   side b       with f
    unsigned* next_tile;                // zero at launch
    int64_t P, NP, stride;
    int V, K, by_sample;
    int min_it, max_it, freq;  // max_it % freq == 0
    double tol;
};

struct SigChangeDrawArgs {
    const double* __restrict__ Ha0;  // [NP][K] the tied fit's exposures of every listed problem, where the observed launch left them
    const double* __restrict__ Hb0;  // [NP][K]
    const double* __restrict__ W;    // [K][V]
    const double* __restrict__ Xa;   // [N][V] the clipped counts: a row's trial count is sum_v (uint32) X[n, v]
    const double* __restrict__ Xb;   // [N][V]
    const int* __restrict__ pair_n;  // [NP]
    const int* __restrict__ pair_s;  // [NP]
    double* __restrict__ out;        // [draws][NP][2][V]
    int64_t NP;
    int V, K;
    uint32_t key0, key1;
    double floor;
    uint32_t first;  // slot 0 of `out` holds draw `first`
};

// salnmf_batch.hip (the translation unit of model_draw_kernel): draws first .. first + count - 1 of every listed problem as out[count][NP][2][V]
void sigchange_launch_draw(const double* Ha0, const double* Hb0, const double* W, const double* Xa, const double* Xb, const int* pair_n,
                           const int* pair_s, double* out, int64_t NP, int V, int K, uint64_t seed, double floor, int first, int count,
                           hipStream_t stream);

#ifdef SALNMF_GOF_KERNELS  // salnmf_batch.hip: after salnmf_gof.h
// One workgroup per (problem, side, draw): blockIdx.x = 2 problem + side, blockIdx.y = draw - a.first.  model_draw_kernel's body with
// the side's own tied exposure row, the side's own total and the stream word of (s, side).
__global__ void __launch_bounds__(RESAMPLE_BLOCK) sigchange_draw_kernel(SigChangeDrawArgs a) {
    const int64_t j = blockIdx.x >> 1;
    const uint32_t side = blockIdx.x & 1u;
    const int n = a.pair_n[j];
    model_draw_row((side ? a.Hb0 : a.Ha0) + (size_t)j * a.K, a.W, nullptr, (side ? a.Xb : a.Xa) + (size_t)n * a.V,
                   a.out + (((size_t)blockIdx.y * a.NP + j) * 2 + side) * a.V, a.V, a.K, a.key0, a.key1,
                   SIGCHANGE_STREAM + 2u * (uint32_t)a.pair_s[j] + side, (uint32_t)n, blockIdx.y + a.first, a.floor);
}
#endif  // SALNMF_GOF_KERNELS

#ifdef SALNMF_REFIT_KERNELS  // salnmf_refit.hip: after salnmf_assign.h

// The value the partner lane (lane ^ 1) holds: quad_perm:[1,0,3,2] on the two halves.  Every lane of the wave is active.
__device__ __forceinline__ int partner_int(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ double partner_double(double v) {
    return __hiloint2double(partner_int(__double2hiint(v)), partner_int(__double2loint(v)));
}

// F = c_a u_a + c_b u_b, evaluated as (u_a + u_b) / 2 + ((c_a - c_b) / 2) (u_a - u_b): the same number since c_a + c_b = 1, and in
// this form two identities hold to the bit.  Exchanging the samples leaves it: the sum commutes, and both factors of the product
// change sign.  And with u_a == u_b it is u_a, whatever c_a is: the product is zero and the halved sum is exact -- so two samples
// with the same shares (x_b = m x_a) keep their free fits in the tied solve and their statistic is 0.0.  The rounded products of
// c_a u_a + c_b u_b give the first identity but not the second: 1 / (1 + m) is no float64 number unless m = 1.  Every operation is
// rounded on its own: the plain operators under the pragma, as salnmf_gof.h's mul_then_add (the toolchain's __dmul_rn / __dadd_rn
// are inline functions of the plain operators, compiled under the default contraction mode, and fuse once inlined).
__device__ __forceinline__ double tied_factor(double ca, double ua, double cb, double ub) {
#pragma clang fp contract(off)
    const double mean = 0.5 * (ua + ub);
    const double lean = 0.5 * (ca - cb);
    const double tilt = lean * (ua - ub);
    return mean + tilt;
}

template <int KT>
__global__ void __launch_bounds__(BLOCK) sigchange_kernel(SigChangeArgs a) {
    constexpr int KP = 16 * KT;
    constexpr int NW = (KT + 1) / 2;  // 32-bit words of a signature set
    __shared__ double Wl[KP * WS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c16 = lane & 15, q = lane >> 4;
    const int side = c16 & 1;  // 0: the column holds sample a, 1: sample b; the partner column is c16 ^ 1
    const int V = a.V, K = a.K;
    solve_stage_w<KT>(Wl, a.W, K, V, tid);
    const int64_t ntiles = (a.P + 7) / 8;
    const double* wp = Wl + q * WS + c16;
    const double* wu = Wl + c16 * WS + q;

    for (;;) {
        const int64_t tile = solve_take_tile(a.next_tile, lane);
        if (tile >= ntiles) break;
        const int64_t p = tile * 8 + (c16 >> 1);
        const int64_t row = p < a.P ? p : a.P - 1;
        const int n = a.pair_n[row % a.NP];
        const int s = a.pair_s[row % a.NP];
        // a column pair past the end of the list is finished from the start: it recomputes the last problem's first step and
        // stores nothing
        const int64_t off = (a.by_sample ? (int64_t)n : row) * a.stride;
        double x[VT][4];
        const double t = solve_load_row((side ? a.Xb : a.Xa) + off, V, q, x);
        const double tp = partner_double(t);
        const double ta = side ? tp : t, tb = side ? t : tp;
        const double ca = ta / (ta + tb), cb = tb / (ta + tb);
        unsigned act[NW];
        const int nc = solve_candidate_words<NW>(K, a.cand, (int64_t)n * NW, act);
        d4 h[KT];
        auto start = [&]() {
            const double h0 = t / (double)nc;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) h[kt][r] = ((act[kt >> 1] >> ((16 * kt + 4 * r + q) & 31)) & 1u) ? h0 : 0.0;
        };
        start();
        int mode = p < a.P ? 0 : 3;  // 0: the free solve, 1: latched, waiting for the partner, 2: the tied solve, 3: finished
        bool fresh = false;          // the solve has just started: its iteration-0 test is due
        int itl = 0;
        double prev = 0.0, ff = 0.0;  // ff: the column's free divergence

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
                const double curp = partner_double(cur);
                const double cura = side ? curp : cur, curb = side ? cur : curp;
                const double obj = mode == 2 ? cura + curb : cur;  // (one rounded sum of two moved values: nothing to contract)
                bool stop = false;
                int cv = 0;
                if ((mode == 0 || mode == 2) && (fresh || !repass)) {
                    stop = solve_stop(itl, prev, obj, a.min_it, a.max_it, a.tol, cv);
                    prev = obj;
                }
                fresh = false;
                if (__any(stop)) {  // (uniform)
                    const double ffp = partner_double(ff);
                    if (stop && mode == 2) {  // both columns of the problem, with the same bits
                        if (a.f) solve_store_column<KT>((side ? a.Hb0 : a.Ha0) + p * K, h, K, q);
                        if (q == 0 && side == 0) {
                            const double fa = ff, fb = ffp;
                            a.stat[p] = (cura - fa) + (curb - fb);
                            a.nit[3 * p + 2] = itl;
                            if (a.f) a.f[4 * p + 2] = cura, a.f[4 * p + 3] = curb, a.conv[3 * p + 2] = cv;
                        }
                        mode = 3;
                    }
                    if (stop && mode == 0) {
                        if (a.f) solve_store_column<KT>((side ? a.Hb : a.Ha) + p * K, h, K, q);
                        if (q == 0) {
                            a.nit[3 * p + side] = itl;
                            if (a.f) a.f[4 * p + side] = cur, a.conv[3 * p + side] = cv;
                        }
                        ff = cur;
                        mode = 1;
                    }
                }
                const int modep = partner_int(mode);
                if (mode == 1 && modep == 1) {  // both free solves are latched: the tied solve's cold start, in both columns
                    start();
                    mode = 2, itl = 0, fresh = true;
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
            const bool tied = __any(mode == 2);  // (uniform)
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double uf = u[kt][r];
                    if (tied) {  // every lane moves; the columns of a tied problem keep F at row s
                        const double up = partner_double(uf);
                        const double F = tied_factor(ca, side ? up : uf, cb, side ? uf : up);
                        uf = (mode == 2 && 16 * kt + 4 * r + q == s) ? F : uf;
                    }
                    const double hn = clip_lo(h[kt][r] * uf, kEps);
                    h[kt][r] = ((mode & 1) || h[kt][r] == 0.0) ? h[kt][r] : hn;
                }
            ++itl;
        }
    }
}
#endif  // SALNMF_REFIT_KERNELS

}  // namespace salnmf
