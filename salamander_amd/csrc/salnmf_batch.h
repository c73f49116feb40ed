// KLNMFSweep on the device (salnmf_batch.hip, include/salnmf.h: salnmf_batch_*): many independent KLNMF models of at most
// 16 signatures on ONE count matrix or on bootstrap resamples of it, one workgroup per model.
//
// Layout (one batch = one device, one uploaded X and R >= 0 resamples of it, "datasets" -1 and 0 .. R - 1):
//   X    [Np][96]       the uploaded matrix, clipped and padded as an engine holds it (salnmf_kernels.h)
//   xlx  [Np][16]       its x-only KL constants (the forward pass's mode 0), once per upload of X
//   Xr   [R][Np][96], xlxr [R][Np][16]   the resamples in the same layout (salnmf_resample.h writes them in place)
//        or, after salnmf_batch_split, 2 F slots: train split f in slot f, test split f in slot F + f (salnmf_split.h)
//   every member reads ONE dataset, through the X / xlx pointers of its BatchMember (the uploaded X until
//   salnmf_batch_set_dataset says otherwise)
//   per member m:  W [K_m][V], H [Np][16] (pad columns 0, pad rows 1 -- an engine's H for K <= 16), G [K_m][V] (the last
//                  step's reduced numerator, what the small kernel leaves behind), objective partials [fgrid] and an arrival
//                  counter of the in-launch sum
// The step calls the same body as the single-model small-cohort kernel (salnmf_small.hip: small_kl_body), and the objective /
// per-sample divergences call the same body as forward_kernel's modes 0 / 1 (salnmf_forward_kernel.h: forward_body) with the
// grid an engine of this shape uses (forward_grid): every member gets the bits a single engine computes for it.
#pragma once
#include "salnmf_launch.h"

namespace salnmf {

struct BatchMember {
    double* W;  // [K][V]
    double* H;  // [Np][16]
    double* G;  // [K][V]
    int K;
    const double* X;    // [Np][96] the member's dataset
    const double* xlx;  // [Np][16] and its constants
};

// one launch of the batched step: workgroup i runs nsteps steps of member active[i] with n_given[i] given signatures
struct SmallBatchArgs {
    const BatchMember* __restrict__ members;
    const int* __restrict__ active;   // [n_active]
    const int* __restrict__ n_given;  // [n_active]
    int V, ntiles, nsteps;
    // per-sample weights (salnmf_batch_set_weights), a table beside the members that only the weighted kernel reads:
    // entries 2 m and 2 m + 1 are member m's w_kl and w_lhalf as an engine holds them ([Np], pad rows 1 / 0), or null
    const double* const* __restrict__ weights;
};
// The first n_plain entries of the lists are members without weights and go through the unweighted kernel, the n_weighted
// entries behind them through the weighted instantiation (small_kl_body<..., WTS = true>): at most two launches.
int launch_small_kl_batch(const SmallBatchArgs& a, int n_plain, int n_weighted, hipStream_t stream);

}  // namespace salnmf
