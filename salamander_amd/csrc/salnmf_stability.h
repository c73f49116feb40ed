// Signature stability of a sweep: match the signatures of all members of one K to each other, form consensus signatures and
// score them by their silhouettes (include/salnmf.h: salnmf_batch_stability, salnmf_signature_stability; DESIGN.md
// section 12, "Stability").
//
// A group is M >= 2 members of K <= 16 signatures over V <= 96 features plus one error value per member.  One workgroup
// runs one group from start to end:
//   u[m][i]   = row i of member m / its Euclidean norm                     (scratch [16][96] per member, pads zero)
//   anchor    = the member of smallest error (lowest index on ties), c = u[anchor]
//   round t:    for every member the 16 x 16 tile c . u[m]^T (24 v_mfma_f64_16x16x4, contraction over the 96 features), the
//               costs D[j][i] = 1 - c[j].u[m][i], and the optimal assignment p[m] of member rows to centroids;
//               s[j] = sum_m u[m][p[m][j]];  stop when no p[m] changed, else c[j] = s[j] / |s[j]|
//   silhouette: the same tile against the unnormalised sums s -- the mean cosine distance of a unit vector to a set of unit
//               vectors is linear in the set's sum
// The assignment is the shortest-augmenting-path (Hungarian) solve with the 16 columns of a member on 16 lanes, four members
// per wave: row potentials live on the lane of their row, column potentials, slack, predecessor and the matched row on the
// lane of their column; every loop has a trip count that depends on K alone, so the whole kernel is free of divergent
// barriers.  The cluster sums are taken by one thread per entry (j, v), over the members in ascending order: the bits do not
// depend on the launch geometry or on timing, and nothing is accumulated with atomics.
#pragma once
#include "salnmf_kernels.h"

namespace salnmf {

constexpr int STAB_K = 16;                  // signatures per member, at most
constexpr int STAB_LD = WS;                 // LDS row stride of the centroids and the cluster sums
constexpr int STAB_TS = 17;                 // LDS row stride of a 16 x 16 tile
constexpr int STAB_PER_WAVE = 4;            // members a wave solves side by side
constexpr int STAB_PER_PASS = WAVES * STAB_PER_WAVE;

struct StabGroup {
    int K, M, first;  // members first .. first + M - 1 of the launch's member table
};

struct StabArgs {
    const StabGroup* __restrict__ groups;     // [gridDim.x]
    const double* const* __restrict__ src;    // [T] each member's signatures, [K][ld]
    const double* __restrict__ err;           // [T]
    int ld, V, max_rounds;
    double* u;                                // [T][16][96] scratch: the unit rows
    double* xx;                               // [T][16] scratch: u[m][i] . u[m][i]
    int* assign;                              // [T][16] p[m][j]
    double *a, *b, *sil;                      // [T][16]
    double* consensus;                        // [G][16][96]
    double* cluster;                          // [G][16] cluster_stability
    double* score;                            // [G][2] stability_mean, stability_min
    int* rounds;                              // [G][2] n_rounds, converged
};

// sum over the 16 lanes of a row of lanes, the same bits in all of them
__device__ __forceinline__ double stab_sum16(double v) {
    v += __shfl_xor(v, 8, 16);
    v += __shfl_xor(v, 4, 16);
    v += __shfl_xor(v, 2, 16);
    v += __shfl_xor(v, 1, 16);
    return v;
}

// L . um^T for L [16][STAB_LD] in LDS and um [16][96] in memory: entry [row = (lane >> 4) + 4 reg][col = lane & 15] in
// register reg (the lane maps of salnmf_kernels.h)
__device__ __forceinline__ d4 stab_tile(const double* L, const double* __restrict__ um, int lane) {
    const int r = lane & 15, q = lane >> 4;
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int s = 0; s < VSTEPS; ++s) acc = mfma(L[r * STAB_LD + 4 * s + q], um[r * VMAX + 4 * s + q], acc);
    return acc;
}

// The optimal assignment of a K x K cost tile (rows: centroids, columns: member rows), columns on the 16 lanes of a row of
// lanes.  Returns the centroid matched to this lane's column (-1 on a pad lane).  Rows are added one at a time; for row r the
// alternating tree grows by one column per iteration and reaches a free column after at most r + 1 of them, so both loops
// run r + 1 times for every member and a member that is through idles.
__device__ __forceinline__ int stab_assign(const double* cost, int K, int j) {
    constexpr double kInf = 1e300;
    const bool col = j < K;
    double u = 0.0, v = 0.0;  // potential of row j, of column j
    int pcol = -1;            // the row matched to column j
    for (int r = 0; r < K; ++r) {
        double minv = kInf;
        int way = -1, i0 = r, j0 = -1, jend = -1;
        bool used = false, rowin = j == r, done = false;
        for (int it = 0; it <= r; ++it) {
            const double ui0 = __shfl(u, i0, 16);
            const double cur = cost[i0 * STAB_TS + j] - ui0 - v;
            const bool open = col && !used;
            if (!done && open && cur < minv) {
                minv = cur;
                way = j0;
            }
            double delta = open ? minv : kInf;
            int j1 = j;
#pragma unroll
            for (int mask = 8; mask > 0; mask >>= 1) {
                const double ov = __shfl_xor(delta, mask, 16);
                const int oj = __shfl_xor(j1, mask, 16);
                if (ov < delta || (ov == delta && oj < j1)) {
                    delta = ov;
                    j1 = oj;
                }
            }
            const int pj1 = __shfl(pcol, j1, 16);
            if (!done) {
                if (rowin) u += delta;
                if (used)
                    v -= delta;
                else
                    minv -= delta;
                j0 = j1;
                if (j == j1) used = true;
                if (pj1 < 0) {
                    done = true;
                    jend = j1;
                } else {
                    i0 = pj1;
                    if (j == pj1) rowin = true;
                }
            }
        }
        // augment along the predecessors, from the free column back to row r
        int jc = jend;
        for (int it = 0; it <= r; ++it) {
            const int jp = __shfl(way, jc < 0 ? 0 : jc, 16);
            const int pp = __shfl(pcol, jp < 0 ? 0 : jp, 16);
            if (jc >= 0) {
                if (j == jc) pcol = jp < 0 ? r : pp;
                jc = jp;
            }
        }
    }
    return pcol;
}

__global__ void __launch_bounds__(BLOCK) stability_kernel(StabArgs p) {
    __shared__ double C[STAB_K * STAB_LD];                               // centroids
    __shared__ double S[STAB_K * STAB_LD];                               // cluster sums
    __shared__ double tile[STAB_PER_PASS * STAB_K * STAB_TS];            // one 16 x 16 tile per member of a pass
    __shared__ int perm[STAB_PER_PASS * STAB_K];
    __shared__ double red[STAB_K];
    __shared__ int flag[2];                                              // anchor | a permutation changed
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, sub = tid >> 4;  // column of the row of lanes, row of lanes of the workgroup (0 .. 15)
    const StabGroup g = p.groups[blockIdx.x];
    const int K = g.K, M = g.M, V = p.V;
    const int passes = (M + STAB_PER_PASS - 1) / STAB_PER_PASS;
    double* U = p.u + (size_t)g.first * STAB_K * VMAX;
    double* XX = p.xx + (size_t)g.first * STAB_K;
    int* P = p.assign + (size_t)g.first * STAB_K;
    double* tl = tile + sub * STAB_K * STAB_TS;  // this row of lanes' member of the pass
    int* pm = perm + sub * STAB_K;

    // unit rows: one row of lanes per signature, the 16 rows of a member per trip
    for (int m = 0; m < M; ++m) {
        const double* w = p.src[g.first + m];
        double x[VT], ss = 0.0;
#pragma unroll
        for (int c = 0; c < VT; ++c) {
            const int v = j + 16 * c;
            x[c] = (sub < K && v < V) ? w[(size_t)sub * p.ld + v] : 0.0;
            ss += x[c] * x[c];
        }
        const double norm = sqrt(stab_sum16(ss));
        double uu = 0.0;
#pragma unroll
        for (int c = 0; c < VT; ++c) {
            x[c] = sub < K ? x[c] / norm : 0.0;
            uu += x[c] * x[c];
            U[((size_t)m * STAB_K + sub) * VMAX + j + 16 * c] = x[c];
        }
        uu = stab_sum16(uu);
        if (j == 0) XX[m * STAB_K + sub] = uu;
    }
    if (tid == 0) {
        int best = 0;
        for (int m = 1; m < M; ++m)
            if (p.err[g.first + m] < p.err[g.first + best]) best = m;
        flag[0] = best;
    }
    __syncthreads();
    for (int e = tid; e < STAB_K * VMAX; e += BLOCK) {
        const int i = e / VMAX, v = e - i * VMAX;
        C[i * STAB_LD + v] = U[((size_t)flag[0] * STAB_K + i) * VMAX + v];
        S[i * STAB_LD + v] = 0.0;
    }
    __syncthreads();

    int n_rounds = 0, converged = 0;
    for (int t = 1; t <= p.max_rounds; ++t) {
        if (tid == 0) flag[1] = t == 1;
        __syncthreads();
        for (int pass = 0; pass < passes; ++pass) {
            for (int q = 0; q < STAB_PER_WAVE; ++q) {  // (wave-uniform)
                const int m = pass * STAB_PER_PASS + wave * STAB_PER_WAVE + q;
                if (m >= M) break;
                const d4 acc = stab_tile(C, U + (size_t)m * STAB_K * VMAX, lane);
                double* dst = tile + (wave * STAB_PER_WAVE + q) * STAB_K * STAB_TS;
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[((lane >> 4) + 4 * r) * STAB_TS + j] = 1.0 - acc[r];
            }
            pm[j] = j < K ? -1 : j;
            __syncthreads();
            const int m = pass * STAB_PER_PASS + sub;
            const int pc = stab_assign(tl, K, j);
            if (pc >= 0 && pc < K && j < K) pm[pc] = j;
            __syncthreads();
            // A tile of non-finite costs may leave rows and columns unmatched (never one of finite costs).  Every lane
            // stored its own column, so the entries that are set differ and as many columns as rows are left: the
            // unmatched rows take them in ascending order.  p[m] is a permutation whatever the input, and a row that
            // is not finite reaches the sums and the scores of a cluster instead of dropping out of them.
            if (j == 0) {
                unsigned taken = 0;
                for (int r = 0; r < K; ++r)
                    if (pm[r] >= 0) taken |= 1u << pm[r];
                int c = 0;
                for (int r = 0; r < K; ++r)
                    if (pm[r] < 0) {
                        while (c < K - 1 && (taken >> c & 1u)) ++c;
                        pm[r] = c;
                        if (c < K - 1) ++c;
                    }
            }
            __syncthreads();
            if (m < M) {
                if (t > 1 && j < K && P[m * STAB_K + j] != pm[j]) flag[1] = 1;
                P[m * STAB_K + j] = pm[j];
            }
            __syncthreads();
        }
        n_rounds = t;
        if (!flag[1]) {
            converged = 1;
            break;
        }
        // cluster sums, members in ascending order
        for (int e = tid; e < K * VMAX; e += BLOCK) {
            const int c = e / VMAX, v = e - c * VMAX;
            double s = 0.0;
            for (int m = 0; m < M; ++m) s += U[((size_t)m * STAB_K + P[m * STAB_K + c]) * VMAX + v];
            S[c * STAB_LD + v] = s;
        }
        __syncthreads();
        if (t == p.max_rounds) break;
        if (tid < K) {
            double ss = 0.0;
            for (int v = 0; v < VMAX; ++v) ss += S[tid * STAB_LD + v] * S[tid * STAB_LD + v];
            red[tid] = sqrt(ss);
        }
        __syncthreads();
        for (int e = tid; e < K * VMAX; e += BLOCK) {
            const int c = e / VMAX, v = e - c * VMAX;
            C[c * STAB_LD + v] = S[c * STAB_LD + v] / red[c];
        }
        __syncthreads();
    }

    // silhouettes: x . s[j'] for every point x = u[m][p[m][j]] is column p[m][j] of the tile s . u[m]^T
    double* A = p.a + (size_t)g.first * STAB_K;
    double* B = p.b + (size_t)g.first * STAB_K;
    double* Z = p.sil + (size_t)g.first * STAB_K;
    for (int pass = 0; pass < passes; ++pass) {
        for (int q = 0; q < STAB_PER_WAVE; ++q) {
            const int m = pass * STAB_PER_PASS + wave * STAB_PER_WAVE + q;
            if (m >= M) break;
            const d4 acc = stab_tile(S, U + (size_t)m * STAB_K * VMAX, lane);
            double* dst = tile + (wave * STAB_PER_WAVE + q) * STAB_K * STAB_TS;
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[((lane >> 4) + 4 * r) * STAB_TS + j] = acc[r];
        }
        __syncthreads();
        const int m = pass * STAB_PER_PASS + sub;
        if (m < M) {
            double a = 0.0, b = __builtin_nan(""), z = 0.0;
            if (j < K) {
                const int i = P[m * STAB_K + j];
                a = 1.0 - (tl[j * STAB_TS + i] - XX[m * STAB_K + i]) / (double)(M - 1);
                for (int c = 0; c < K; ++c) {
                    const double d = 1.0 - tl[c * STAB_TS + i] / (double)M;
                    if (c != j && !(d >= b)) b = d;  // (b starts as NaN: the first other cluster always replaces it)
                }
                z = K == 1 ? 1.0 : (b - a) / (a > b ? a : b);
            }
            A[m * STAB_K + j] = a;
            B[m * STAB_K + j] = j < K ? b : 0.0;
            Z[m * STAB_K + j] = z;
        }
        __syncthreads();
    }

    // consensus signatures and the scores
    if (tid < STAB_K) {
        double rs = 0.0, z = 0.0;
        if (tid < K) {
            for (int v = 0; v < VMAX; ++v) rs += S[tid * STAB_LD + v];
            for (int m = 0; m < M; ++m) z += Z[m * STAB_K + tid];
            z /= (double)M;
        }
        red[tid] = rs;
        p.cluster[(size_t)blockIdx.x * STAB_K + tid] = z;
    }
    __syncthreads();
    for (int e = tid; e < STAB_K * VMAX; e += BLOCK) {
        const int c = e / VMAX, v = e - c * VMAX;
        p.consensus[(size_t)blockIdx.x * STAB_K * VMAX + e] = c < K ? S[c * STAB_LD + v] / red[c] : 0.0;
    }
    if (tid == 0) {
        double sum = 0.0, lo = p.cluster[(size_t)blockIdx.x * STAB_K];
        for (int c = 0; c < K; ++c) {
            const double z = p.cluster[(size_t)blockIdx.x * STAB_K + c];
            sum += z;
            if (lo == lo && !(z >= lo)) lo = z;  // (a NaN wins and stays: it is reported, not skipped)
        }
        p.score[2 * blockIdx.x] = sum / (double)K;
        p.score[2 * blockIdx.x + 1] = lo;
        p.rounds[2 * blockIdx.x] = n_rounds;
        p.rounds[2 * blockIdx.x + 1] = converged;
    }
}

inline void launch_stability(const StabArgs& a, int n_groups, hipStream_t stream) {
    hipLaunchKernelGGL(stability_kernel, dim3((unsigned)n_groups), dim3(BLOCK), 0, stream, a);
}

}  // namespace salnmf
