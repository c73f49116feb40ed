// Could the presence test have seen signature s in this sample?  Detection power and limit per (sample, tested signature)
// (include/salnmf.h: salnmf_signature_power), on the pairs, the null fits h0 and the [B][pairs] null
// statistics that the presence test (salnmf_presence.h) leaves on the device.
//
// LEVEL l plants the tested signature s of a pair at the share pi_l of the pair's null fit h0 (K doubles, exactly 0.0 at s):
//   S0 = sum_k h0[k], from 0.0 in ascending k over all K;  c_l = 1.0 - pi_l, one rounded subtraction;
//   Hp[k] = c_l h0[k] for k != s,  Hp[s] = pi_l S0 -- each one rounded product, no fused multiply-add.
// pi = 0 gives h0 back bit for bit (1.0 h0[k], and 0.0 S0 = 0.0 = h0[s]).
//
// Alternative draw a of (pair, level l) is the model draw of salnmf_gof.h, steps 1-6, from row (l, pair) of the planted
// exposures with the sample's own total, under the Philox counter (q, 0x50570000 + s, n, a): a fifth stream family, "PW" in
// the upper half of the second word.  The level is NOT in the counter: all levels of a pair share their random numbers, so a
// level's draws do not depend on where it stands among the shares or on what other shares are asked for, and two levels with
// equal planted rows have equal draws.  A draw depends on (seed, n, s, a) and on its planted row, and on nothing else.
//
// Every draw goes through presence_kernel as it stands (two cold solves, by_sample = 0): the chunk buffer is [count][NP][V] with
// r = l A + a running over the rows, so pair = row mod NP holds.
//
// Reduction, one thread per (pair, level) walking a and, inside, b, both ascending: e_a = #{b : t_b >= t*_a} over the pair's B
// null statistics (false for a NaN on either side); draw a is DETECTED iff t*_a is not NaN and e_a <= max_exceed;
// n_detected counts them; alt_mean is the sum of t*_a from 0.0 in ascending a, divided by A.
// The solves of the alternative draws are presence_kernel launches (salnmf_presence.h, on the solve_* pieces of salnmf_refit.h),
// issued by the same draw-and-solve loop as the presence test's null draws (salnmf_refit.hip: pair_draw_solve).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace salnmf {

constexpr uint32_t POWER_STREAM = 0x50570000u;  // "PW" << 16: the second counter word of a block is this plus the tested signature
constexpr int POWER_MAX_SHARES = 64;
constexpr int POWER_MAX_DRAWS = 65536;  // per share

struct PowerPlantArgs {
    const double* __restrict__ H0;      // [NP][K] the null fits, where the observed launch left them
    const int* __restrict__ pair_s;     // [NP]
    const double* __restrict__ shares;  // [L]
    double* __restrict__ Hp;            // [L][NP][K]
    int64_t NP;
    int K, L;
};

struct PowerDrawArgs {
    const double* __restrict__ Hp;   // [L][NP][K]
    const double* __restrict__ W;    // [K][V]
    const double* __restrict__ X;    // [N][V] the clipped counts: row n's trial count is sum_v (uint32) X[n, v]
    const int* __restrict__ pair_n;  // [NP]
    const int* __restrict__ pair_s;  // [NP]
    double* __restrict__ out;        // [rows][NP][V]
    int64_t NP;
    int V, K;
    uint32_t key0, key1;
    double floor;
    uint32_t first;  // slot 0 of `out` holds row r = `first`, r = l A + a
    uint32_t A;
};

struct PowerReduceArgs {
    const double* __restrict__ stat_null;  // [B][NP]
    const double* __restrict__ stat_alt;   // [L A][NP]
    int* __restrict__ n_exceed;            // [L A][NP]
    int* __restrict__ n_detected;          // [L][NP]
    double* __restrict__ alt_mean;         // [L][NP]
    int64_t NP;
    int B, L, A, max_exceed;
};

// salnmf_batch.hip (the translation unit of model_draw_kernel and gof_reduce_kernel)
void power_launch_plant(const PowerPlantArgs& a, hipStream_t stream);
// rows first .. first + count - 1 of every pair as out[count][NP][V]
void power_launch_draw(const double* Hp, const double* W, const double* X, const int* pair_n, const int* pair_s, double* out, int64_t NP, int V, int K,
                       uint64_t seed, double floor, int n_alt_draws, int64_t first, int64_t count, hipStream_t stream);
void power_launch_reduce(const PowerReduceArgs& a, hipStream_t stream);

#ifdef SALNMF_GOF_KERNELS  // salnmf_batch.hip: after salnmf_gof.h
// One thread per (level, pair) walking k twice: the sum, then the row.
__global__ void __launch_bounds__(256) power_plant_kernel(PowerPlantArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.NP * a.L) return;
    const int64_t l = i / a.NP, j = i - l * a.NP;
    const double* h0 = a.H0 + (size_t)j * a.K;
    double* hp = a.Hp + (size_t)i * a.K;
    const int s = a.pair_s[j];
    const double pi = a.shares[l];
    const double c = 1.0 - pi;
    double S0 = 0.0;
    for (int k = 0; k < a.K; ++k) S0 += h0[k];
    for (int k = 0; k < a.K; ++k) hp[k] = k == s ? pi * S0 : c * h0[k];
}

// One workgroup per (pair, row r): model_draw_kernel's body with the planted row of (r / A, pair) and the counter word r % A.
__global__ void __launch_bounds__(RESAMPLE_BLOCK) power_draw_kernel(PowerDrawArgs a) {
    const int64_t j = blockIdx.x;
    const int n = a.pair_n[j], s = a.pair_s[j];
    const uint32_t r = blockIdx.y + a.first;
    const uint32_t l = r / a.A, d = r - l * a.A;
    model_draw_row(a.Hp + ((size_t)l * a.NP + j) * a.K, a.W, nullptr, a.X + (size_t)n * a.V, a.out + ((size_t)blockIdx.y * a.NP + j) * a.V, a.V, a.K,
                   a.key0, a.key1, POWER_STREAM + (uint32_t)s, (uint32_t)n, d, a.floor);
}

// One thread per (level, pair): see the top of the file.
__global__ void __launch_bounds__(256) power_reduce_kernel(PowerReduceArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.NP * a.L) return;
    const int64_t l = i / a.NP, j = i - l * a.NP;
    int detected = 0;
    double sum = 0.0;
    for (int d = 0; d < a.A; ++d) {
        const size_t o = ((size_t)l * a.A + d) * a.NP + j;
        const double t = a.stat_alt[o];
        int e = 0;
        for (int b = 0; b < a.B; ++b) e += a.stat_null[(size_t)b * a.NP + j] >= t ? 1 : 0;
        a.n_exceed[o] = e;
        detected += (t == t && e <= a.max_exceed) ? 1 : 0;
        sum += t;
    }
    a.n_detected[i] = detected;
    a.alt_mean[i] = sum / (double)a.A;
}
#endif  // SALNMF_GOF_KERNELS

}  // namespace salnmf
