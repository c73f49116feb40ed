// Count vectors drawn on the device from a FITTED negative-binomial model (include/salnmf.h: salnmf_draw_nb_counts,
// salnmf_nb_goodness_of_fit): the gamma-Poisson draw.  Row n of draw b, exposures h (K doubles), signatures
// W (K x V, rows of sum one), dispersion alpha = alpha_n, is UNCONDITIONAL -- its total varies -- and is built in four steps:
//   1. P_v = sum_k h_k W[k, v], from 0.0 in ascending k by mul_then_add (salnmf_gof.h: step 1 of section 16's contract);
//   2. lambda_v = g_v (P_v / alpha), g_v ~ Gamma(shape alpha, scale 1), one lane per channel v < V (a channel with P_v / alpha == 0
//      draws nothing and has lambda_v = 0): Marsaglia-Tsang on the shape a' = alpha (alpha >= 1) or alpha + 1 (alpha < 1), with
//      d = a' - 1/3 and c = 1 / sqrt(9 d) computed on the host; the normal by the polar method; no squeeze step; for alpha < 1 the
//      result times exp(log(u4) / alpha)                                                                        (nb_gamma);
//   3. Lambda = sum_v lambda_v from 0.0 in ascending v and T ~ Poisson(Lambda), both by lane 0: below 10 by counting exponentials,
//      from 10 on by Hoermann's PTRS with this file's loggam                                                    (nb_poisson);
//   4. T trials over the table of lambda_v / Lambda: steps 3, 5 and 6 of section 16's contract (40-bit weights by __ddiv_rn, the
//      64-bit cum, upper_cell64, the __umul64hi placement, the LDS histogram of ones).
// Generator: philox4x32_10 (salnmf_resample.h), key = (seed & 0xffffffff, seed >> 32), counter (q, stream, n, b); the second
// counter word is the fifth family 0x4E420000 ("NB" << 16): + v for channel v's gamma attempts, + 0xFF00 for the total's, + 0xFFFF
// for the placement blocks.  A uniform takes 53 bits of two words, u(lo, hi) = ((double)(hi << 21 | lo >> 11) + 0.5) 2^-53 (the sum
// is rounded to nearest even from 2^52 on, so u lies in [2^-54, 1]).  Gamma attempt q of channel v: block 2q gives u1 = u(o0, o1),
// u2 = u(o2, o3); block 2q + 1, generated only if the attempt reaches the acceptance test, gives u3 = u(o0, o1), u4 = u(o2, o3).
// Total, Lambda < 10: uniform j is u(o0, o1) (j even) or u(o2, o3) (j odd) of block j >> 1.  PTRS attempt q: block q, U = u(o0, o1)
// - 0.5, V = u(o2, o3).  Placement: block q gives trials 2q and 2q + 1 as in section 16.
//
// Every floating-point operation is +, -, x under `#pragma clang fp contract(off)`, an explicit __builtin_fma, __ddiv_rn,
// __dsqrt_rn, floor, a conversion, or log_pos (salnmf_kernels.h); nb_exp and nb_loggam are written here from those, so that
// tests/_nbdraw_ref.py repeats every one of them.  Every loop is bounded: 64 attempts per gamma, 128 exponentials, 64 PTRS
// attempts.  A row that exhausts one of them, or whose Lambda is 2^31 or more, is written as zeros and counted into *failed.
//
// log_pos operands (all pass log_operand_ok: positive, normal, between 2^-962 and 2^963):
//   u3, u4, the exponentials' u, PTRS' V      in [2^-54, 1];
//   s = a1^2 + a2^2, tested 0 < s < 1          a = 2u - 1 is exact and a multiple of 2^-53, so s >= 2^-106;
//   v = (1 + c x)^3, tested v > 0              |x| <= sqrt(-2 log s) < 12.2 and c <= 6^-1/2: 1 + c x is one fma, at least 2^-110
//                                              in magnitude when it is not 0, and below 6; v in [2^-330, 216];
//   Lambda in [10, 2^31); invalpha in (1.12, 1.33]; a / us^2 + b >= b > 8.9 and <= 2^108 a + b, a < 2912 (Lambda < 2^31, us >= 2^-54);
//   x0 in [7, 2^32 + 1]; the shift's product in [1, 720].
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "salnmf_gof.h"

namespace salnmf {

constexpr uint32_t NB_STREAM = 0x4E420000u;        // "NB" << 16: + v, the gamma attempts of channel v (v < 96)
constexpr uint32_t NB_STREAM_TOTAL = 0x4E42FF00u;  // the total's attempts
constexpr uint32_t NB_STREAM_PLACE = 0x4E42FFFFu;  // the placement blocks
constexpr int NB_GAMMA_ATTEMPTS = 64;
constexpr int NB_EXPONENTIALS = 128;  // P(Poisson(10) >= 128) < 2^-300
constexpr int NB_PTRS_ATTEMPTS = 64;
constexpr double NB_MAX_MEAN = 16777216.0;  // 2^24: the host refuses a row with sum_v P_v above it

struct NbDrawArgs {
    const double* __restrict__ H;      // [N][K] the exposures
    const double* __restrict__ W;      // [K][V] the signatures, rows of sum one
    const double* __restrict__ alpha;  // [N] the dispersions
    const double* __restrict__ gd;     // [N] d = a' - 1/3, a' = alpha >= 1 ? alpha : alpha + 1
    const double* __restrict__ gc;     // [N] c = 1 / sqrt(9 d)
    double* __restrict__ out;          // [draws][N][V]
    unsigned* failed;                  // one word: rows that were written as zeros because a loop ran out or Lambda >= 2^31
    int64_t N;
    int V, K;
    uint32_t key0, key1;
    double floor;    // entries are max(count, floor): 0 (raw) or SALNMF_EPSILON
    uint32_t first;  // slot 0 of `out` holds draw `first`
};

// salnmf_batch.hip (the translation unit that includes salnmf_resample.h): draws first .. first + count - 1 of the series of
// `seed` as out[count][N][V]
void nb_launch_draw(const double* H, const double* W, const double* alpha, const double* gd, const double* gc, double* out, unsigned* failed, int64_t N,
                    int V, int K, uint64_t seed, double floor, int first, int count, hipStream_t stream);

#ifdef SALNMF_NBDRAW_KERNELS  // salnmf_batch.hip alone compiles the kernel (after salnmf_resample.h, salnmf_kernels.h and salnmf_gof.h's kernels)

__device__ __forceinline__ double nb_uniform(uint32_t lo, uint32_t hi) {
#pragma clang fp contract(off)
    return ((double)((uint64_t)hi << 21 | lo >> 11) + 0.5) * 0x1p-53;
}

// exp(t) for t <= 0 (and the few ulps above 0 that log_pos(1.0) / alpha can be): 0 below -708; k = the integer nearest to
// t / ln 2 (by the 1.5 x 2^52 constant), r = t - k ln2_hi - k ln2_lo (the first product is exact: ln2_hi has 32 bits, |k| <= 1022),
// the Taylor polynomial of degree 13 in Horner form, and an exact scale by 2^k (k >= -1021: the result is normal)
__device__ __forceinline__ double nb_exp(double t) {
#pragma clang fp contract(off)
    if (t < -708.0) return 0.0;
    const double kd = (t * 1.44269504088896338700e+00 + 0x1.8p52) - 0x1.8p52;
    double r = __builtin_fma(-kd, 6.93147180369123816490e-01, t);
    r = __builtin_fma(-kd, 1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = __builtin_fma(p, r, 1.0 / 479001600.0);
    p = __builtin_fma(p, r, 1.0 / 39916800.0);
    p = __builtin_fma(p, r, 1.0 / 3628800.0);
    p = __builtin_fma(p, r, 1.0 / 362880.0);
    p = __builtin_fma(p, r, 1.0 / 40320.0);
    p = __builtin_fma(p, r, 1.0 / 5040.0);
    p = __builtin_fma(p, r, 1.0 / 720.0);
    p = __builtin_fma(p, r, 1.0 / 120.0);
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return p * __hiloint2double((1023 + (int)kd) << 20, 0);
}

// log Gamma(x) for an integer-valued x >= 1: the Stirling series at x0 = x + n, n = 7 - x below 7 and 0 otherwise, less the
// logarithm of the product x (x + 1) .. (x + n - 1) (an integer of at most 720, exact)
__device__ __forceinline__ double nb_loggam(double x, const double* __restrict__ tab) {
#pragma clang fp contract(off)
    const double nd = x < 7.0 ? 7.0 - x : 0.0;
    const double x0 = x + nd;
    double prod = 1.0;
    for (int i = 0; i < 6; ++i)
        if ((double)i < nd) prod = prod * (x + (double)i);
    const double x2 = __ddiv_rn(1.0, x0 * x0);
    double g = -1.392432216905900e+00;
    g = __builtin_fma(g, x2, 1.796443723688307e-01);
    g = __builtin_fma(g, x2, -2.955065359477124e-02);
    g = __builtin_fma(g, x2, 6.410256410256410e-03);
    g = __builtin_fma(g, x2, -1.917526917526918e-03);
    g = __builtin_fma(g, x2, 8.417508417508418e-04);
    g = __builtin_fma(g, x2, -5.952380952380952e-04);
    g = __builtin_fma(g, x2, 7.936507936507937e-04);
    g = __builtin_fma(g, x2, -2.777777777777778e-03);
    g = __builtin_fma(g, x2, 8.333333333333333e-02);
    const double tail = __builtin_fma(x0 - 0.5, log_pos(x0, tab), -x0);
    double gl = (__ddiv_rn(g, x0) + 9.189385332046727e-01) + tail;  // 0.5 log(2 pi)
    if (nd > 0.0) gl = gl - log_pos(prod, tab);
    return gl;
}

// g ~ Gamma(alpha, 1) for channel `stream - NB_STREAM` of row n of draw b; false when NB_GAMMA_ATTEMPTS attempts were all rejected
__device__ __forceinline__ bool nb_gamma(double alpha, double d, double c, uint32_t stream, uint32_t n, uint32_t b, uint32_t key0, uint32_t key1,
                                         const double* __restrict__ tab, double* g) {
#pragma clang fp contract(off)
    for (uint32_t q = 0; q < (uint32_t)NB_GAMMA_ATTEMPTS; ++q) {
        uint32_t o[4];
        philox4x32_10(2u * q, stream, n, b, key0, key1, o);
        const double a1 = __builtin_fma(2.0, nb_uniform(o[0], o[1]), -1.0);
        const double a2 = __builtin_fma(2.0, nb_uniform(o[2], o[3]), -1.0);
        const double s = a1 * a1 + a2 * a2;
        if (!(s > 0.0 && s < 1.0)) continue;
        const double x = a1 * __dsqrt_rn(__ddiv_rn(-2.0 * log_pos(s, tab), s));
        const double t = __builtin_fma(c, x, 1.0);
        const double v = (t * t) * t;
        if (!(v > 0.0)) continue;
        philox4x32_10(2u * q + 1u, stream, n, b, key0, key1, o);
        const double rhs = __builtin_fma(d, log_pos(v, tab), __builtin_fma(-d, v, __builtin_fma(0.5, x * x, d)));
        if (!(log_pos(nb_uniform(o[0], o[1]), tab) < rhs)) continue;
        double out = d * v;
        if (alpha < 1.0) out = out * nb_exp(__ddiv_rn(log_pos(nb_uniform(o[2], o[3]), tab), alpha));
        *g = out;
        return true;
    }
    *g = 0.0;
    return false;
}

// T ~ Poisson(lam) for row n of draw b, 0 < lam < 2^31 (one lane); false when a loop ran out or T does not fit 32 bits
__device__ __forceinline__ bool nb_poisson(double lam, uint32_t n, uint32_t b, uint32_t key0, uint32_t key1, const double* __restrict__ tab, uint32_t* T) {
#pragma clang fp contract(off)
    *T = 0;
    uint32_t o[4];
    if (lam < 10.0) {
        double s = 0.0;
        uint32_t count = 0;
        for (uint32_t j = 0; j < (uint32_t)NB_EXPONENTIALS; ++j) {
            if (!(j & 1u)) philox4x32_10(j >> 1, NB_STREAM_TOTAL, n, b, key0, key1, o);
            s = s - log_pos((j & 1u) ? nb_uniform(o[2], o[3]) : nb_uniform(o[0], o[1]), tab);
            if (!(s < lam)) {
                *T = count;
                return true;
            }
            ++count;
        }
        return false;
    }
    const double slam = __dsqrt_rn(lam), loglam = log_pos(lam, tab);
    const double bb = __builtin_fma(2.53, slam, 0.931);
    const double aa = __builtin_fma(0.02483, bb, -0.059);
    const double invalpha = 1.1239 + __ddiv_rn(1.1328, bb - 3.4);
    const double vr = 0.9277 - __ddiv_rn(3.6224, bb - 2.0);
    const double log_invalpha = log_pos(invalpha, tab), shifted = lam + 0.43;
    for (uint32_t q = 0; q < (uint32_t)NB_PTRS_ATTEMPTS; ++q) {
        philox4x32_10(q, NB_STREAM_TOTAL, n, b, key0, key1, o);
        const double U = nb_uniform(o[0], o[1]) - 0.5, Vv = nb_uniform(o[2], o[3]);
        const double us = 0.5 - __builtin_fabs(U);
        if (!(us > 0.0)) continue;
        const double k = __builtin_floor(__builtin_fma(__ddiv_rn(2.0 * aa, us) + bb, U, shifted));
        bool accept = us >= 0.07 && Vv <= vr;
        if (!accept) {
            if (k < 0.0 || (us < 0.013 && Vv > us)) continue;
            const double lhs = (log_pos(Vv, tab) + log_invalpha) - log_pos(__ddiv_rn(aa, us * us) + bb, tab);
            // k >= 2^32 > 2 lam is rejected outright: the test would (its right side is below -0.38 lam there, its left side above -200)
            if (!(k < 4294967296.0)) continue;
            accept = lhs <= __builtin_fma(k, loglam, -lam) - nb_loggam(k + 1.0, tab);
        }
        if (accept) {
            if (!(k >= 0.0 && k < 4294967296.0)) return false;
            *T = (uint32_t)k;
            return true;
        }
    }
    return false;
}

// Row n of draw b by one workgroup of RESAMPLE_BLOCK lanes
__device__ __forceinline__ void nb_draw_row(const double* __restrict__ h, const double* __restrict__ W, double alpha, double d, double c,
                                            double* __restrict__ out, unsigned* failed, int V, int K, uint32_t key0, uint32_t key1, uint32_t n, uint32_t b,
                                            double floor) {
    __shared__ __attribute__((aligned(16))) double tab[LOGTAB_DOUBLES];
    __shared__ double hs[GOF_KMAX];
    __shared__ double lambda[GOF_VMAX];
    __shared__ uint64_t cum[GOF_VMAX];
    __shared__ uint32_t hist[GOF_VMAX];
    __shared__ uint32_t trials;
    __shared__ uint32_t bad;
    static_assert(RESAMPLE_BLOCK == LOGTAB_N, "one table entry per lane");
    const int tid = threadIdx.x;
    stage_logtab(tab, tid);
    if (tid < K) hs[tid] = h[tid];
    if (tid < V) hist[tid] = 0;
    if (tid == 0) bad = 0;
    __syncthreads();
    if (tid < V) {
        double p = 0.0;
        for (int k = 0; k < K; ++k) p = mul_then_add(p, hs[k], W[k * V + tid]);
        const double scale = __ddiv_rn(p, alpha);
        double g = 0.0;
        if (scale != 0.0 && !nb_gamma(alpha, d, c, NB_STREAM + (uint32_t)tid, n, b, key0, key1, tab, &g)) bad = 1;
        lambda[tid] = mul_then_add(0.0, g, scale);
    }
    __syncthreads();
    if (tid == 0) {  // the sum, the total and the table in one fixed order
        double L = 0.0;
        for (int v = 0; v < V; ++v) L += lambda[v];
        uint32_t T = 0;
        bool ok = bad == 0;
        if (ok && L > 0.0 && L < __builtin_inf()) {
            ok = L < 2147483648.0 && nb_poisson(L, n, b, key0, key1, tab, &T);
            if (!ok) T = 0;
        }
        if (!ok) atomicAdd(failed, 1u);
        if (T) {
            uint64_t s = 0;
            for (int v = 0; v < V; ++v) cum[v] = s += (uint64_t)(__ddiv_rn(lambda[v], L) * 0x1p40);
        }
        trials = T;
    }
    __syncthreads();
    const uint32_t T = trials;
    if (T) {
        const uint64_t M = cum[V - 1];
        const uint32_t nblocks = (T >> 1) + (T & 1);
        for (uint32_t q = tid; q < nblocks; q += RESAMPLE_BLOCK) {
            uint32_t o[4];
            philox4x32_10(q, NB_STREAM_PLACE, n, b, key0, key1, o);
            atomicAdd(&hist[upper_cell64(__umul64hi((uint64_t)o[1] << 32 | o[0], M), cum, V)], 1u);
            if (2 * (uint64_t)q + 1 < T) atomicAdd(&hist[upper_cell64(__umul64hi((uint64_t)o[3] << 32 | o[2], M), cum, V)], 1u);
        }
    }
    __syncthreads();
    if (tid < V) out[tid] = clipped_count(hist[tid], floor);
}

// One workgroup per (row, draw): blockIdx.x = row, blockIdx.y = draw - a.first.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) nb_draw_kernel(NbDrawArgs a) {
    const int64_t n = blockIdx.x;
    nb_draw_row(a.H + (size_t)n * a.K, a.W, a.alpha[n], a.gd[n], a.gc[n], a.out + ((size_t)blockIdx.y * a.N + n) * a.V, a.failed, a.V, a.K, a.key0, a.key1,
                (uint32_t)n, blockIdx.y + a.first, a.floor);
}
#endif  // SALNMF_NBDRAW_KERNELS

}  // namespace salnmf
