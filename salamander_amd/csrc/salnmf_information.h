// The information matrix of a sample's exposures at the fit, its inverse, and what the inverse says about confounding
// (include/salnmf.h: salnmf_exposure_covariance).
//
// Per sample, with x the clipped counts, h the exposures as supplied and A the active signatures:
//   p_v = max(sum_k W[k, v] h_k, EPSILON)                      over all k
//   d_v = x_v / p_v^2 (observed) or 1 / p_v (expected)
//   J[k, l] = sum_v W[k, v] W[l, v] d_v                        k, l in A
//   C = D^-1/2 J D^-1/2, D = diag(J);  C = L L^T in the natural order, no pivoting;  C^-1 = L^-T L^-1
//
// information_kernel<KT>: one workgroup of four waves per CU takes samples off a ticket.  W [16 KT][WS] sits in LDS once per
// workgroup, zero padded as the refit kernels keep it (rows k >= K and columns v >= V are 0), a second array Cl [16 KT][16 KT + 1]
// holds the sample's matrix through every stage:
//   1. p and d, one feature per thread, plain FMAs over k ascending;
//   2. the lower-triangle 16 x 16 tiles of J by v_mfma_f64_16x16x4, W the A operand and d * W the B operand, both from LDS,
//      KT (KT + 1) / 2 tiles of ceil(V / 4) k-steps dealt round robin to the four waves.  Only entries with row >= col are kept:
//      the two halves of a diagonal tile round differently, and everything below reads the lower triangle alone;
//   3. the scaling to C; an inactive or pad row and column becomes that of the identity, so every trip count below depends on K
//      alone and every barrier sits in uniform control flow;
//   4. a right-looking Cholesky in place (two barriers per column), every thread following the pivots in registers: the smallest
//      squared pivot over the active k, and `singular` at the first one <= min_pivot (a NaN counts as singular).  The factorisation
//      runs to the end either way -- on guarded pivots -- and a singular sample's results are replaced by NaN;
//   5. L^-1 in place, columns from the last to the first, row i by thread i (one barrier per column);
//   6. (C^-1)_kk = sum_m (L^-1)[m, k]^2, then every (C^-1)_kl, l < k, as a correlation into the strict UPPER triangle of Cl: one
//      number per unordered pair, so the correlation matrix is symmetric bit for bit;
//   7. per k the largest |corr| over the active l != k in ascending l (the smallest index wins a tie), and the stores.
// Pads never reach an output: pad columns of W are 0 and d is 0 there, pad rows k >= K are never read past stage 3.
// All stores are plain vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace salnmf {

constexpr int INFO_KMAX = 96;

struct InfoArgs {
    const double* __restrict__ X;     // [N][V] clipped
    const double* __restrict__ W;     // [K][V]
    const double* __restrict__ H;     // [N][K]
    const uint8_t* __restrict__ act;  // [N][K]
    double* __restrict__ se;          // [N][K]
    double* __restrict__ infl;        // [N][K]
    double* __restrict__ info;        // [N][K]
    double* __restrict__ maxc;        // [N][K]
    int* __restrict__ conf;           // [N][K]
    double* __restrict__ minp;        // [N]
    int* __restrict__ sing;           // [N]
    int* __restrict__ nact;           // [N]
    double* __restrict__ corr;        // null, or [count][K][K]: the chunk's correlations
    unsigned* next;                   // zero at launch: the ticket
    int64_t first, count;             // the launch's samples: first .. first + count - 1
    int V, K, expected;
    double min_pivot;
};

#ifdef SALNMF_INFORMATION_KERNELS  // salnmf_information.hip alone compiles the kernel (it includes salnmf_kernels.h first)

template <int KT>
__global__ void __launch_bounds__(BLOCK) information_kernel(InfoArgs a) {
    constexpr int KP = 16 * KT, CS = KP + 1;
    __shared__ double Wl[KP * WS];
    __shared__ double Cl[KP * CS];
    __shared__ double dl[VMAX], hl[KP], jd[KP], sc[KP], ld[KP], xd[KP], vd[KP];
    __shared__ int actl[KP];
    __shared__ unsigned ticket;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, q = lane >> 4;
    const int ti = tid >> 4, tc = tid & 15;
    const int V = a.V, K = a.K;
    const int VS = (V + 3) / 4;
    const double nan = __builtin_nan("");
    for (int i = tid; i < KP * WS; i += BLOCK) {
        const int k = i / WS, v = i - k * WS;
        Wl[i] = (k < K && v < V) ? a.W[k * V + v] : 0.0;
    }

    for (;;) {
        if (tid == 0) ticket = atomicAdd(a.next, 1u);
        __syncthreads();
        const unsigned t = ticket;  // (uniform)
        if ((int64_t)t >= a.count) break;
        const int64_t n = a.first + (int64_t)t;
        if (tid < KP) {
            hl[tid] = tid < K ? a.H[n * K + tid] : 0.0;
            actl[tid] = (tid < K && a.act[n * K + tid]) ? 1 : 0;
        }
        __syncthreads();

        // 1. the model mean and the weights
        if (tid < VMAX) {
            double d = 0.0;
            if (tid < V) {
                double p = 0.0;
                for (int k = 0; k < K; ++k) p = __builtin_fma(Wl[k * WS + tid], hl[k], p);
                p = p < kEps ? kEps : p;
                d = a.expected ? 1.0 / p : a.X[n * V + tid] / (p * p);
            }
            dl[tid] = d;
        }
        int nact = 0;
        for (int k = 0; k < K; ++k) nact += actl[k];
        __syncthreads();

        // 2. the lower-triangle tiles of J
        for (int tile = wave; tile < KT * (KT + 1) / 2; tile += WAVES) {
            int it = 0, jt = tile;
            while (jt > it) jt -= ++it;
            const double* wa = Wl + (16 * it + c16) * WS + q;
            const double* wb = Wl + (16 * jt + c16) * WS + q;
            d4 acc = {0, 0, 0, 0};
            for (int s = 0; s < VS; ++s) acc = mfma(wa[4 * s], dl[4 * s + q] * wb[4 * s], acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * it + q + 4 * r, col = 16 * jt + c16;
                if (row >= col) Cl[row * CS + col] = acc[r];
            }
        }
        __syncthreads();

        // 3. C = D^-1/2 J D^-1/2, identity off the active set
        if (tid < KP) {
            const double j = Cl[tid * CS + tid];
            jd[tid] = j;
            sc[tid] = actl[tid] ? 1.0 / sqrt(j) : 0.0;
        }
        __syncthreads();
        for (int i = ti; i < KP; i += 16)
            for (int c = tc; c <= i; c += 16) {
                double v = (actl[i] && actl[c]) ? Cl[i * CS + c] * sc[i] * sc[c] : 0.0;
                if (c == i) v = 1.0;
                Cl[i * CS + c] = v;
            }
        __syncthreads();

        // 4. C = L L^T in place; L's diagonal goes to ld
        double minp = __builtin_inf();
        bool sing = false;
        for (int j = 0; j < K; ++j) {
            const double piv = Cl[j * CS + j];
            if (actl[j] && !sing) {
                if (!(piv > a.min_pivot)) sing = true, minp = piv;
                else minp = piv < minp ? piv : minp;
            }
            const double l = sqrt(piv > 0.0 ? piv : 1.0);
            for (int i = j + 1 + tid; i < K; i += BLOCK) Cl[i * CS + j] = Cl[i * CS + j] / l;
            if (tid == 0) ld[j] = l;
            __syncthreads();
            for (int i = j + 1 + ti; i < K; i += 16) {
                const double lij = Cl[i * CS + j];
                for (int c = j + 1 + tc; c <= i; c += 16) Cl[i * CS + c] = __builtin_fma(-lij, Cl[c * CS + j], Cl[i * CS + c]);
            }
            __syncthreads();
        }

        // 5. X = L^-1 in place, its diagonal in xd: X[i][j] = -(sum_{j < m <= i} X[i][m] L[m][j]) / L[j][j]
        if (tid < K) xd[tid] = 1.0 / ld[tid];
        __syncthreads();
        for (int j = K - 1; j >= 0; --j) {
            const int i = tid;
            double val = 0.0;
            if (i > j && i < K) {
                double acc = 0.0;
                for (int m = j + 1; m < i; ++m) acc = __builtin_fma(Cl[i * CS + m], Cl[m * CS + j], acc);
                acc = __builtin_fma(xd[i], Cl[i * CS + j], acc);
                val = -acc * xd[j];
            }
            __syncthreads();  // column j of L has been read by every row
            if (i > j && i < K) Cl[i * CS + j] = val;
        }
        __syncthreads();

        // 6. the diagonal of C^-1 = X^T X, then every pair's correlation into the upper triangle
        if (tid < K) {
            double acc = xd[tid] * xd[tid];
            for (int m = tid + 1; m < K; ++m) acc = __builtin_fma(Cl[m * CS + tid], Cl[m * CS + tid], acc);
            vd[tid] = acc;
        }
        __syncthreads();
        for (int k = ti; k < K; k += 16)
            for (int l = tc; l < k; l += 16) {
                double acc = xd[k] * Cl[k * CS + l];
                for (int m = k + 1; m < K; ++m) acc = __builtin_fma(Cl[m * CS + k], Cl[m * CS + l], acc);
                Cl[l * CS + k] = acc / sqrt(vd[k] * vd[l]);
            }
        __syncthreads();

        // 7. the results
        const bool ok = !sing && nact > 0;
        if (tid < K) {
            const int k = tid;
            const bool on = ok && actl[k];
            int best = -1;
            double bv = -1.0;
            if (on)
                for (int l = 0; l < K; ++l)
                    if (l != k && actl[l]) {
                        const double c = fabs(l < k ? Cl[l * CS + k] : Cl[k * CS + l]);
                        if (c > bv) bv = c, best = l;
                    }
            a.se[n * K + k] = on ? sqrt(vd[k] / jd[k]) : nan;
            a.infl[n * K + k] = on ? vd[k] : nan;
            a.info[n * K + k] = on ? jd[k] : nan;
            a.maxc[n * K + k] = best >= 0 ? bv : nan;
            a.conf[n * K + k] = best;
        }
        if (tid == 0) {
            a.minp[n] = nact > 0 ? minp : nan;
            a.sing[n] = sing ? 1 : 0;
            a.nact[n] = nact;
        }
        if (a.corr) {
            double* out = a.corr + (size_t)t * K * K;
            for (int k = ti; k < K; k += 16)
                for (int l = tc; l < K; l += 16) {
                    double v = nan;
                    if (ok && actl[k] && actl[l]) v = k == l ? 1.0 : (l < k ? Cl[l * CS + k] : Cl[k * CS + l]);
                    out[k * K + l] = v;
                }
        }
        __syncthreads();  // the next sample rewrites hl, actl and Cl
    }
}

#endif  // SALNMF_INFORMATION_KERNELS

}  // namespace salnmf
