// Refit of exposures to FIXED signatures (include/salnmf.h: salnmf_refit_exposures).
//
// With W fixed the samples decouple: a call with R bootstrap resamples is N (R + 1) independent problems of K unknowns that
// share one W.  Problem = one row x of a count matrix (the counts themselves or a resample of them), clipped to EPSILON:
//   h_k = (sum_v x_v) / K;   step: wh = h W, a = x / wh, h_k <- max(h_k sum_v W[k, v] a_v, EPSILON)    (_utils_klnmf.py:258-264)
//   objective: the row's KL divergence as forward mode 1 computes it (salnmf_forward_kernel.h), at iteration 0 and at every
//   multiple of conv_test_freq; stop at the first test at or after min_iterations with |prev - cur| / |prev| < tol (a NaN
//   comparison is false), else at max_iterations, not converged.  A stopped problem's h is latched.
//
// refit_kernel: W [KP][WS] sits in LDS once per workgroup (zero padded: rows k >= K and columns v >= V are 0).  A wave owns a
// tile of 16 problems -- problem = lane column c16 -- for all its steps, then takes the next tile from an atomic counter.
// Everything is computed TRANSPOSED, so that both products take W as the A operand (from LDS) and the wave's own data as the
// B operand straight from the previous product's accumulator registers (salnmf_kernels.h: register `reg` of a D tile is the
// B operand of k-step `reg` of a product that contracts over D's row index).  No LDS transpose, no per-wave LDS at all:
//   P^T [v][n] = sum_k W[k][v] h^T[k][n]     6 output tiles, 4 KT k-steps each;  B = h^T, registers of the U^T tiles
//   a^T [v][n] = x^T / P^T                   in the accumulator registers (0 in the pad feature rows)
//   U^T [k][n] = sum_v W[k][v] a^T[v][n]     KT output tiles, 24 k-steps each;   B = a^T, registers of the P^T tiles
//   h^T <- max(h^T U^T, EPSILON)             in the accumulator layout (0 in the pad signature rows, which W's zero rows
//                                            keep out of P anyway)
// Column c16 of a B operand only ever reaches column c16 of D: a problem's numbers never meet another problem's, so its
// result cannot depend on its neighbours in the tile, on the tile it lands in, or on when the others stop.  A wave leaves its
// tile when all 16 problems are latched; every branch and trip count is wave-uniform (ballots).  Lane columns beyond the end
// of the list recompute the last problem and store nothing.
//
// What this kernel shares with assign_kernel, presence_kernel and profile_kernel is written once, as the solve_* pieces in
// front of it: the W fill, the tile ticket, the row load, the update factors, the store of an h column, the candidate words and
// the stop rule.  A further analysis on this family writes its own loop and state machine around them.
// A kernel calls a piece only where the call leaves its registers as they were (profiles/refit_pieces/README.md): these
// kernels fill the register file, and where a piece moved the allocation the kernel keeps the statements in line.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace salnmf {

constexpr int REFIT_KMAX = 96;
constexpr int REFIT_MAX_QUANTILES = 16;
constexpr int REFIT_SORT_MAX = 1024;  // resamples the reduction sorts in one pass (LDS); more are refused
constexpr int REFIT_SORT_BLOCK = 256;

// salnmf_batch.hip (the translation unit of resample_counts_kernel): the counts as uint32 or the resampler's refusal, and
// resamples first .. first + count - 1 of the series of `seed`, written compactly as out[count][N][V], clipped to EPSILON
int refit_check_counts(const double* X, int64_t N, int V, std::vector<uint32_t>& counts);
void refit_launch_resample(const uint32_t* counts, double* out, int64_t N, int V, uint64_t seed, int first, int count, hipStream_t stream);

struct RefitArgs {
    const double* __restrict__ X;  // [P][V] compact, clipped
    const double* __restrict__ W;  // [K][V]
    double* __restrict__ H;        // [P][K]
    double* __restrict__ err;      // [P]
    int* __restrict__ nit;         // [P]
    int* __restrict__ conv;        // [P]
    unsigned* next_tile;           // zero at launch: the tile list's head
    int64_t P;                     // problems
    int V, K;
    int min_it, max_it, freq;
    double tol;
};

struct RefitReduceArgs {
    const double* __restrict__ H;  // [R][N][K]
    double* __restrict__ quant;    // [Q][N][K]
    double* __restrict__ mean;     // [N][K]
    int64_t N;
    int K, R, Q, R2;               // R2: the power of two >= R that is sorted
    int index[REFIT_MAX_QUANTILES];
};

// salnmf_refit.hip (the translation unit of refit_reduce_kernel): red.index as check_resamples left it (salnmf_host_kit.h), every
// other member filled here -- the reduction of H [R][N][K] to the mean and the Q order statistics of every (sample, signature)
void refit_launch_reduce(RefitReduceArgs& red, const double* H, double* quant, double* mean, int64_t N, int K, int R, int Q, hipStream_t stream);

#ifdef SALNMF_REFIT_KERNELS  // the tile-solve pieces and refit_kernel, for the units that instantiate tile-solve kernels (salnmf_kernels.h first)

// One problem's KL divergence from the lane's 24 entries (rows v = 16 vt + 4 r + q of column c16): forward mode 1's term
// (salnmf_forward_kernel.h) per entry, the lane's entries in (vt, r) order, then the four q groups by rows_sum -- the same
// bits in all four lanes of the column.
__device__ __forceinline__ double refit_objective(const double (&x)[VT][4], const d4 (&pr)[VT], int V, int q) {
    double acc = 0.0;
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (16 * vt + 4 * r + q < V) {
                const double xv = x[vt][r], pv = pr[vt][r];
                const double xe = (xv == 0.0) ? kEps : xv, pe = (xv == 0.0) ? kEps : pv;
                const double l = (log_operand_ok(xe) && log_operand_ok(pe)) ? log_ratio(xe, pe) : log(xe / pe);
                acc += xe * l - xv + pv;
            }
        asm volatile("" : "+v"(acc));  // four logarithms side by side, one batch after the other: 24 at once cost the step its registers
    }
    return rows_sum(acc);
}

// ---- the pieces of a tile solve.  refit_kernel below, assign_kernel (salnmf_assign.h), presence_kernel (salnmf_presence.h) and
// profile_kernel (salnmf_profile.h) are built from them: each kernel keeps its own loop and its own per-column state machine
// and calls these for what all four do alike.  All are forced inline and hold no state: no LDS but W's, nothing per wave.
// Kept in line where the call moved a kernel's register allocation: the P^T product in all four (as a piece it cost 21 of the
// 30 instantiations 2 to 20 AGPRs, so there is none), the stop rule in refit_kernel, and the W fill, ticket, row load and
// candidate words in profile_kernel.

// W [16 KT][WS] into LDS, zero padded (rows k >= K and columns v >= V are 0), and the barrier after it
template <int KT>
__device__ __forceinline__ void solve_stage_w(double* Wl, const double* W, int K, int V, int tid) {
    for (int i = tid; i < 16 * KT * WS; i += BLOCK) {
        const int k = i / WS, v = i - k * WS;
        Wl[i] = (k < K && v < V) ? W[k * V + v] : 0.0;
    }
    __syncthreads();
}

// The wave's next tile off the list's head (uniform)
__device__ __forceinline__ int64_t solve_take_tile(unsigned* next_tile, int lane) {
    unsigned ticket = 0;
    if (lane == 0) ticket = atomicAdd(next_tile, 1u);
    return (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)ticket);
}

// The lane's 24 entries of its column's row (rows v = 16 vt + 4 r + q, 0 beyond V) -> the row's sum, alike in the column's lanes
__device__ __forceinline__ double solve_load_row(const double* xs, int V, int q, double (&x)[VT][4]) {
    double t = 0.0;
#pragma unroll
    for (int vt = 0; vt < VT; ++vt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = 16 * vt + 4 * r + q;
            x[vt][r] = v < V ? xs[v] : 0.0;
            t += x[vt][r];
        }
    return rows_sum(t);
}

// U^T of a step from its P^T, the update factors at h: wu = Wl + c16 WS + q, A[i = k][v] = W[16 kt + c16][4 s + q]
template <int KT>
__device__ __forceinline__ void solve_update_factors(const double (&x)[VT][4], const d4 (&pr)[VT], const double* wu, int V, int q, d4 (&u)[KT]) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) u[kt] = (d4){0, 0, 0, 0};
#pragma unroll
    for (int vt = 0; vt < VT; ++vt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double av = (16 * vt + 4 * r + q < V) ? div_path(x[vt][r], pr[vt][r]) : 0.0;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) u[kt] = mfma(wu[16 * kt * WS + 4 * (4 * vt + r)], av, u[kt]);
        }
}

// The lane's entries of h into row `dst` of a [P][K] array
template <int KT>
__device__ __forceinline__ void solve_store_column(double* dst, const d4 (&h)[KT], int K, int q) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 16 * kt + 4 * r + q;
            if (k < K) dst[k] = h[kt][r];
        }
}

// A column's candidate set as NW words: all K signatures, or words row .. row + NW - 1 of `cand` -> the members' count
template <int NW>
__device__ __forceinline__ int solve_candidate_words(int K, const unsigned* cand, int64_t row, unsigned (&act)[NW]) {
    int nc = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int m = K - 32 * w;
        act[w] = m >= 32 ? ~0u : m > 0 ? (1u << m) - 1u : 0u;
        if (cand) act[w] &= cand[row + w];
        nc += __popc(act[w]);
    }
    return nc;
}

// The tolerance test of a solve at its iteration itl (a NaN comparison is false)
__device__ __forceinline__ bool solve_converged(int itl, double prev, double cur, int min_it, double tol) {
    return itl > 0 && itl >= min_it && fabs(prev - cur) / fabs(prev) < tol;
}

// The stop rule of a solve whose tests fall on its own iteration count (max_it is a multiple of the test frequency): on the
// tolerance (cv = 1), else at max_it
__device__ __forceinline__ bool solve_stop(int itl, double prev, double cur, int min_it, int max_it, double tol, int& cv) {
    bool stop = false;
    if (solve_converged(itl, prev, cur, min_it, tol)) stop = true, cv = 1;
    if (itl == max_it) stop = true;
    return stop;
}

template <int KT>
__global__ void __launch_bounds__(BLOCK) refit_kernel(RefitArgs a) {
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
                const double cur = refit_objective(x, pr, V, q);
                if (!latched) {
                    if (at_test && it > 0 && it >= a.min_it && fabs(prev - cur) / fabs(prev) < a.tol) latched = true, conv = 1;
                    if (it == a.max_it) latched = true;
                    prev = err = cur;
                    nit = it;
                }
                if (__all(latched)) break;
            }
            d4 u[KT];
            solve_update_factors<KT>(x, pr, wu, V, q, u);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double hn = clip_lo(h[kt][r] * u[kt][r], kEps);
                    h[kt][r] = (latched || 16 * kt + 4 * r + q >= K) ? h[kt][r] : hn;
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
#endif  // SALNMF_REFIT_KERNELS

#ifdef SALNMF_REFIT_REDUCE_KERNEL  // salnmf_refit.hip alone: an ordinary kernel, defined once in the library (refit_launch_reduce)

// One workgroup per sample n: the mean over r of every signature's exposure (thread k, ascending r), then per signature
// the R values sorted in LDS (bitonic, padded with +inf to a power of two) and the order statistics the host asked for.
__global__ void __launch_bounds__(REFIT_SORT_BLOCK) refit_reduce_kernel(RefitReduceArgs a) {
    __shared__ double s[REFIT_SORT_MAX];
    const int tid = threadIdx.x;
    const int64_t n = blockIdx.x;
    const int K = a.K, R = a.R, R2 = a.R2;
    const size_t stride = (size_t)a.N * K;
    for (int k = tid; k < K; k += REFIT_SORT_BLOCK) {
        const double* src = a.H + (size_t)n * K + k;
        double t = 0.0;
        for (int r = 0; r < R; ++r) t += src[(size_t)r * stride];
        a.mean[(size_t)n * K + k] = t / (double)R;
    }
    for (int k = 0; k < K; ++k) {
        for (int r = tid; r < R2; r += REFIT_SORT_BLOCK) s[r] = r < R ? a.H[(size_t)r * stride + (size_t)n * K + k] : __builtin_inf();
        __syncthreads();
        for (int len = 2; len <= R2; len <<= 1)
            for (int d = len >> 1; d > 0; d >>= 1) {
                for (int i = tid; i < R2 / 2; i += REFIT_SORT_BLOCK) {
                    const int lo = 2 * i - (i & (d - 1)), hi = lo + d;  // (hi < R2)
                    const bool up = (lo & len) == 0;
                    const double x = s[lo], y = s[hi];
                    if ((x > y) == up) s[lo] = y, s[hi] = x;
                }
                __syncthreads();
            }
        if (tid < a.Q) a.quant[((size_t)tid * a.N + n) * K + k] = s[a.index[tid]];
        __syncthreads();
    }
}
#endif  // SALNMF_REFIT_REDUCE_KERNEL

}  // namespace salnmf
