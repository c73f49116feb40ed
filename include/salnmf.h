/*
 * salnmf.h -- C ABI of the MI355X-native KL-NMF update engine.
 *
 * The reference (parklab/Salamander @ 2024_10_08) has no FFI: its hot path is a set
 * of NumPy/numba functions called from Python.  This header is therefore the boundary
 * a maintainer would bind (ctypes); each entry point names the
 * reference function (file:line under the reference tree) whose arithmetic it
 * replaces.  Plain pointers and sizes only; no torch / numpy types.
 *
 * Conventions
 *   - All matrices are float64, row-major, in AnnData's storage layout:
 *       X  (n_samples  x n_features)    adata.X
 *       H  (n_samples  x n_signatures)  adata.obsm["exposures"]
 *       W  (n_signatures x n_features)  asignatures.X
 *     (the reference passes the .T views of exactly these buffers,
 *      src/salamander/models/klnmf.py:97-104).
 *   - Every function returns 0 on success, non-zero on failure; the message is
 *     available from salnmf_last_error().  Nothing aborts.
 *   - Host pointers are borrowed for the duration of the call only.  The engine owns
 *     all device memory.  A handle is not re-entrant.
 *   - One engine = one GPU = one shard of the sample axis.
 *
 * Limits of this build (the reference has none; every BASELINE.json configuration fits):
 *   n_features <= 3072, n_signatures <= 512 (salnmf_create: what is available beyond 96 features / 64 signatures),
 *   dim_embeddings <= 64, joint sample solves over at most 4 modalities / 128 signatures.  Anything larger is refused
 *   with a message by salnmf_create / salnmf_corr_configure / salnmf_corr_update_sample_embeddings_multi -- never
 *   silently truncated.  They come from the register / LDS plan of the fused kernel.
 */
#ifndef SALNMF_H
#define SALNMF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct salnmf_engine salnmf_engine;

/* clip floor used everywhere on the path: np.finfo(np.float32).eps as a double
 * (src/salamander/models/_utils_klnmf.py:7). */
#define SALNMF_EPSILON 1.1920928955078125e-07

/* W-tail variants */
#define SALNMF_CLIP_ALL 0       /* update_WH: clip every column, _utils_klnmf.py:341 */
#define SALNMF_CLIP_NON_GIVEN 1 /* update_W: clip only non-given columns, _utils_klnmf.py:215 */

/* device buffers that can be exposed to a caller-side collective (salnmf_device_ptr).
 * G, W, OBJ and RED are compact; X and H are in the engine's padded device layout
 * (X [16*ceil(N/16)][96], H [16*ceil(N/16)][16*ceil(K/16)... see salnmf_kernels.h]). */
#define SALNMF_BUF_G 0    /* (n_signatures x n_features) numerator aux@H.T, local shard */
#define SALNMF_BUF_W 1
#define SALNMF_BUF_H 2
#define SALNMF_BUF_X 3
#define SALNMF_BUF_OBJ 4  /* scalar objective partial of the local shard */
#define SALNMF_BUF_RED 5  /* MvNMF reduction vector: [G (K*V) | rowsums_H (K) | KL (1)] */

const char* salnmf_last_error(void);
int salnmf_version(void);
/* Optional parts compiled into this library: SALNMF_BUILD_PERSISTENT = the persistent multi-step KL kernel
 * (a measured negative; only in builds made with SALNMF_WITH_PERSISTENT=1). */
#define SALNMF_BUILD_PERSISTENT 1
int salnmf_build_flags(void);
int salnmf_device_count(void);

/* Create an engine for a shard of n_samples rows on HIP device `device`.
 * Limits of this build: n_signatures <= 512; n_features <= 3072.  Up to
 * 96 features and 64 signatures (every BASELINE configuration) the whole API is available.  Wider catalogues (SBS-288,
 * SBS-1536, ...) run the KLNMF entry points -- upload / download, salnmf_kl_step (both halves from the old state, as
 * update_WH), salnmf_update_H / _W, the objectives (blocking and queued), salnmf_samplewise_kl, salnmf_reconstruct,
 * per-sample weights -- one 96-feature block of X and W per launch (U = R W^T accumulated over the blocks).  More than 64
 * signatures run the same entry points per chunk of <= 64 signatures: the product H W is accumulated over the chunks by a
 * chain of forward launches, the last of which forms the ratio X / (H W) (or the objective), and the update passes run
 * once per chunk on that ratio.  On feature blocks also: MvNMF (the step in its plain form, salnmf_mv_wide_kernels.h),
 * CorrNMF (its two passes over X block by block; everything else is K- and dim-sized) and the device-side
 * initialisation incl. the separableNMF selection.  On signature chunks also: MvNMF (round 5: the same plain form, its
 * K x K algebra -- Gram matrix, elimination, log det, A and B -- in global memory; mvnmf.py:116-126 has no limit on
 * n_signatures).  Both together (round 5): per feature block the chain over the chunks forms that block's ratio, every chunk
 * runs its numerator pass and its share of U = R W^T on it (accumulated over the blocks); the KLNMF entry points and MvNMF.
 * Sample shards (salnmf_comm_init / salnmf_p2p_connect) of either kind run the KLNMF entry points, the
 * device-side initialisation, MvNMF and -- on feature blocks -- CorrNMF: the numerators of all blocks / chunks cross the
 * ranks in ONE all-reduce of K * V doubles per W update (through RCCL beyond the peer inbox's 16 384 doubles).  The fp32
 * fast mode answers with an error in both cases, and so does CorrNMF on more than 64 signatures.  The device-side
 * initialisation runs everywhere (more than 64 signatures: projection and post-processing chunk by chunk). */
int salnmf_create(int device, int n_features, int64_t n_samples, int n_signatures,
                  salnmf_engine** out);
void salnmf_destroy(salnmf_engine* e);

/* Upload the count matrix.  clip != 0 applies X.clip(EPSILON) on the way, as
 * SignatureNMF._setup_adata does (src/salamander/models/signature_nmf.py:281).
 * Ingest is pinned, chunked and overlapped: the caller's array is copied in 32 MB chunks into two pinned staging
 * buffers by a few host threads, each chunk crosses PCIe by asynchronous DMA and is converted / clipped / padded
 * into the engine's layout by a kernel while the next chunk is being staged.  The typed entry point takes raw count
 * matrices as they come (float32 / int32 / int64 / uint16): the conversion to float64 happens on the device. */
#define SALNMF_F64 0
#define SALNMF_F32 1
#define SALNMF_I32 2
#define SALNMF_I64 3
#define SALNMF_U16 4
int salnmf_upload_X(salnmf_engine* e, const double* X, int clip);
int salnmf_upload_X_typed(salnmf_engine* e, const void* X, int dtype /* SALNMF_F64 ... */, int clip);
int salnmf_upload_W(salnmf_engine* e, const double* W);
int salnmf_upload_H(salnmf_engine* e, const double* H);
/* Per-sample weights (each n_samples long) or NULL to disable
 * (KLNMF._setup_fitting_parameters, klnmf.py:128-153). */
int salnmf_set_weights(salnmf_engine* e, const double* weights_kl, const double* weights_lhalf);
/* normalize_WH's exposure side (utils.py:155-158) + clip, applied lazily: from now on H is read as
 * clip(H * scale[k], EPSILON) by every pass (scale: n_signatures values, the column sums of the raw signatures), and the
 * first pass that rewrites H stores it that way -- the initialisation's 40 MB pass over the exposures disappears into
 * the first update (initialize.py:116-118 with init_method="custom" inside fit). */
int salnmf_set_H_scale(salnmf_engine* e, const double* scale);
int salnmf_download_W(salnmf_engine* e, double* W);
int salnmf_download_H(salnmf_engine* e, double* H);

/* n_steps joint KLNMF updates, device resident: update_WH, _utils_klnmf.py:281-361.
 * The first n_given rows of W are never changed.
 * Opt-in (salnmf_set_persistent, in builds compiled with -DSALNMF_WITH_PERSISTENT): with n_steps >= 2, no per-sample weights and no communicator
 * attached, the steps run in ONE persistent launch (workgroups stay resident; the W tail and its hand-offs happen
 * inside the kernel) -- same bits as step-by-step launches, measured 10 % slower on MI355X, hence off
 * by default.  A wait inside that kernel that gives up (another process holding CUs) is reported by the next
 * synchronising call as an error; the resident state is then invalid. */
int salnmf_kl_step(salnmf_engine* e, int n_steps, int n_given);
/* salnmf_kl_step that keeps the state it starts from: the first step writes the new H / W into second buffers (no
 * copy), which then change roles.  salnmf_kl_rollback returns to the kept state (once, until the next _keep call); the
 * steps it discards may still be running.  For a caller that queues the next block of steps BEFORE it has read the
 * objective that decides convergence (signature_nmf.py:373-380): the decision's host round trip hides behind the block. */
int salnmf_kl_step_keep(salnmf_engine* e, int n_steps, int n_given);
/* Small cohorts: with at most `max_tiles` tiles of 16 samples (default 8 = 128 samples, at most 64), at most 16
 * signatures, no weights, fp64, one device, salnmf_kl_step runs ALL n_steps of a call in ONE launch of ONE workgroup
 * (csrc/salnmf_small.hip: W in LDS, workgroup barriers only) instead of two launches per step: 2.1x / 1.5x the per-step
 * path's rate at 64 / 128 samples.  One workgroup has one CU's matrix pipes, so from 12 tiles on (the reference's own
 * data/pcawg_breast_sbs.csv: 192 samples) the per-step path is as fast; hence the default.  Bit for bit the same W, H as
 * the per-step path at every size (the summation orders are reproduced).  0 turns it off. */
int salnmf_set_small_cohort_tiles(salnmf_engine* e, int max_tiles);
int salnmf_kl_rollback(salnmf_engine* e);
/* The objective (klnmf.py:64-80) of the resident state into slot `slot` of the objective ring (as salnmf_objective_async),
 * then n_steps >= 0 joint updates (keep != 0: as salnmf_kl_step_keep).  This is what SignatureNMF.fit does at every
 * convergence test that does not end the fit (signature_nmf.py:358-385): the first update forms P = H W of exactly the
 * state the objective is about, so -- unweighted, unsharded, n_features <= 96, n_given < n_signatures -- the divergence is
 * evaluated inside that update's launch (one logarithm per entry on top of it) and reduced by a spare workgroup of its
 * W tail; no forward pass of its own.  Otherwise, and for n_steps == 0, the calls named above in sequence.  The value
 * equals salnmf_objective's to rounding (another summation order), not bit for bit. */
int salnmf_kl_step_objective(salnmf_engine* e, int slot, int n_steps, int n_given, int keep);
/* Switch the persistent multi-step launch of salnmf_kl_step on (1) or off (0, the default).  Measurement aid: the
 * default build does not carry that kernel (measured 10 % slower) and refuses on = 1 with an error; build with
 * SALNMF_WITH_PERSISTENT=1 (__graft_entry__.py) to get it. */
int salnmf_set_persistent(salnmf_engine* e, int on);
/* update_H with the current W: _utils_klnmf.py:220-278. */
int salnmf_update_H(salnmf_engine* e);
/* update_W (clip_mode = SALNMF_CLIP_NON_GIVEN): _utils_klnmf.py:164-217. */
int salnmf_update_W(salnmf_engine* e, int n_given, int clip_mode);

/* KLNMF.objective_function: weighted kl_divergence (+ l-half penalty if set),
 * klnmf.py:64-80 and _utils_klnmf.py:11-55.  With a communicator attached the value
 * is all-reduced over the shards. */
int salnmf_objective(salnmf_engine* e, double* out);
/* The same without a host round trip: queue the objective of the resident state into slot `slot` of a device ring
 * (SALNMF_OBJECTIVE_SLOTS entries, pinned host memory the reducing kernel writes directly), read a range of slots later:
 * the read waits for those objectives only, not for work queued behind them.
 * SignatureNMF.fit evaluates the objective every conv_test_freq iterations (signature_nmf.py:373-383) but cannot stop
 * before min_iterations: until then the values are only queued and come back in one read. */
#define SALNMF_OBJECTIVE_SLOTS 256
int salnmf_objective_async(salnmf_engine* e, int slot);
int salnmf_objective_read(salnmf_engine* e, int first, int count, double* out);
/* samplewise_kl_divergence, _utils_klnmf.py:58-97 (unweighted); out has n_samples. */
int salnmf_samplewise_kl(salnmf_engine* e, double* out);
/* H @ W (n_samples x n_features): SignatureNMF.compute_reconstruction,
 * signature_nmf.py:221-224. */
int salnmf_reconstruct(salnmf_engine* e, double* out);

/* MvNMF (src/salamander/models/mvnmf.py).  One call = n_steps times
 * _update_parameters (:197-210): update_H (:162-165), update_W_unconstrained (:37-66),
 * line_search (:69-92).  gamma_inout carries MvNMF._gamma across calls. */
int salnmf_mv_step(salnmf_engine* e, int n_steps, int n_given, double lam, double delta,
                   double* gamma_inout);
/* The pieces of the W step as the reference exposes them (function-level API of mvnmf.py):
 *   salnmf_mv_logdet                  volume_logdet (mvnmf.py:19-24) of the resident W
 *   salnmf_mv_update_W_unconstrained  update_W_unconstrained (:37-66) from the resident (X, W, H) -> Wunc_out [K][V];
 *                                     the resident state is not changed.  Accuracy: the reference's closed-form root
 *                                     subtracts root - b, so an entry with b = rowsum_H - 4 lam A > 0 is good to
 *                                     eps * kappa only, kappa ~ rowsum_H^2 / (4 lam B G) (1e6 .. 1e12 on count data); that
 *                                     is a property of mvnmf.py's formula, which this library restates operation for operation
 *   salnmf_mv_line_search             line_search (:69-92) from the resident (X, W, H) with the caller's
 *                                     W_unconstrained [K][V]: leaves the accepted W and the rescaled H resident, updates gamma */
int salnmf_mv_logdet(salnmf_engine* e, double delta, double* out);
int salnmf_mv_update_W_unconstrained(salnmf_engine* e, int n_given, double lam, double delta, double* Wunc_out);
int salnmf_mv_line_search(salnmf_engine* e, double lam, double delta, double* gamma_inout, const double* Wunc);
/* salnmf_mv_step that also returns MvNMF.objective_function (mvnmf.py:149-156) of the state it leaves behind: the line
 * search of the last step has evaluated exactly that (its accepted f, mvnmf.py:82-89), so a fit loop that tests
 * convergence after a block of steps (signature_nmf.py:373-380) needs no salnmf_mv_objective call -- one forward pass, one
 * log det and one host round trip less per test.  Equal to salnmf_mv_objective's value to rounding.
 * more_follows != 0: the caller expects to go on with another salnmf_mv_step* call (same delta, n_given).  Inside a call
 * every step but the last already runs the first half of its successor speculatively while the host waits for the
 * line-search scalars; with more_follows the last step does so too and the engine keeps that half step across the calls
 * (W is the accepted trial, H already the successor's update).  Any other entry point first steps back to the plain
 * accepted state (no kernel: the pre-update exposures are still there), so results never depend on the flag. */
/* MvNMF steps of an unsharded engine are QUEUED AHEAD of the host (default): per step a tail launch and one pass over the
 * samples (update_H with the trial + the numerator of the next W step: fused_kernel<.., MVJ>); the line-search decision
 * of step i (mvnmf.py:84) is taken on the device, in the prologue of step i + 1's tail; the host reads a flag and the
 * scalars once per call and resolves a rejected first trial on the classic path.  0 = the classic form: one host decision
 * per step, two passes over the samples.  Same results bit for bit. */
int salnmf_set_mv_queued(salnmf_engine* e, int on);
/* The update passes copy W (38 KB at K = 50) into every workgroup's LDS once per launch.  Default (1): by LDS-DMA
 * (global_load_lds_dwordx4, no registers) where n_features == 96 and W is 16-byte aligned; 0: through registers (the
 * form of rounds 1-4; any other layout takes it anyway).  Same results bit for bit (W is copied, not computed). */
int salnmf_set_w_dma(salnmf_engine* e, int on);
/* Workgroups of the update passes' launches: min(compute units, ceil(tiles / 4)), four waves each.  With it a caller can
 * tell which form the leftover round of a shape takes (csrc/salnmf_fused_kernel.h: the pairing rule). */
int salnmf_fused_grid(salnmf_engine* e, int* grid);
int salnmf_mv_step_objective(salnmf_engine* e, int n_steps, int n_given, double lam, double delta,
                             double* gamma_inout, double* objective_out, int more_follows);
/* only MvNMF._update_W (:190-195) / only _update_H (= salnmf_update_H) for the
 * reference's single-step tests (tests/test_mvnmf.py:70-76). */
int salnmf_mv_update_W(salnmf_engine* e, int n_given, double lam, double delta,
                       double* gamma_inout);
/* kl_divergence_penalized, mvnmf.py:27-34. */
int salnmf_mv_objective(salnmf_engine* e, double lam, double delta, double* out);

/* ---- Correlated NMF, dense pieces.  The exposure matrix is not a free
 * parameter but exp(signature scaling + sample scaling + <signature embedding, sample
 * embedding>) (src/salamander/models/corrnmf.py:66-77).  The engine keeps the scalings and
 * embeddings next to X / W / H; H holds the exposures.  Both families of embedding solves
 * (scipy.optimize.minimize(method="Newton-CG") in the reference, _utils_corrnmf.py:354-410) run on
 * the device: salnmf_corr_update_signature_embeddings and salnmf_corr_update_sample_embeddings.
 * One CorrNMFDet._update_parameters (corrnmf_det.py:157-169) is the sequence
 *   update_sample_scalings, compute_exposures, compute_aux, update_signature_scalings,
 *   update_signature_embeddings, update_sample_embeddings, [variance: host scalar], update_signatures. */
#define SALNMF_CORR_SIGNATURE_SCALINGS 0   /* [n_signatures]                       */
#define SALNMF_CORR_SAMPLE_SCALINGS 1      /* [n_samples]                          */
#define SALNMF_CORR_SIGNATURE_EMBEDDINGS 2 /* [n_signatures][dim_embeddings]       */
#define SALNMF_CORR_SAMPLE_EMBEDDINGS 3    /* [n_samples][dim_embeddings]          */
#define SALNMF_CORR_AUX 4                  /* [n_samples][n_signatures] = aux.T    */
/* Allocate the CorrNMF state for embeddings of dimension dim_embeddings (1..64); all zero. */
int salnmf_corr_configure(salnmf_engine* e, int dim_embeddings);
int salnmf_corr_upload(salnmf_engine* e, int which, const double* src);
int salnmf_corr_download(salnmf_engine* e, int which, double* dst);
/* update_sample_scalings, _utils_corrnmf.py:141-179 (CorrNMFDet.update_sample_scalings,
 * corrnmf_det.py:32-44). */
int salnmf_corr_update_sample_scalings(salnmf_engine* e);
/* compute_exposures, _utils_corrnmf.py:11-25: overwrites H. */
int salnmf_corr_compute_exposures(salnmf_engine* e);
/* compute_aux, _utils_corrnmf.py:28-52: aux[n][k] = H[n][k] * sum_v W[k][v] X[n][v] / (HW)[n][v]
 * from the current X, W, H.  The same pass leaves the reduced numerator of update_W in
 * SALNMF_BUF_G for salnmf_corr_update_signatures. */
int salnmf_corr_compute_aux(salnmf_engine* e);
/* update_signature_scalings, _utils_corrnmf.py:103-138, from the aux buffer. */
int salnmf_corr_update_signature_scalings(salnmf_engine* e);
/* CorrNMFDet.update_signatures (corrnmf_det.py:71-86) = update_W, _utils_klnmf.py:164-217, with
 * the numerator of the last salnmf_corr_compute_aux (W and the exposures are unchanged in
 * between in CorrNMFDet._update_parameters). */
int salnmf_corr_update_signatures(salnmf_engine* e, int n_given);
/* CorrNMFDet.update_sample_embeddings (corrnmf_det.py:115-141): one Newton-CG solve per sample
 * (update_embedding, _utils_corrnmf.py:354-410, objective :182-239, gradient :242-293, Hessian
 * :296-351) from the current sample embeddings, using the aux buffer, both scalings and the
 * signature embeddings on the device.  maxiter <= 0 selects SciPy's default (200 * dim);
 * CorrNMFDet passes 3.  status_out (n_samples ints, or NULL) receives per solve 0 = converged,
 * 1 = iteration limit, 2 = line search failed, 3 = CG failed (SciPy's warnflag values).
 * The arithmetic restates SciPy's `_minimize_newtoncg` + `_line_search_wolfe12`
 * (salamander_amd/csrc/salnmf_newtoncg.h). */
int salnmf_corr_update_sample_embeddings(salnmf_engine* e, double variance, int maxiter,
                                         int* status_out);
/* MultimodalCorrNMF.update_sample_embeddings (mmcorrnmf.py:398-428): the sample embeddings are
 * shared by the modalities, so one solve per sample sees the signatures (embeddings, scalings, aux)
 * of all of them and that modality's sample scaling per term.  engines[i] is modality i (1..4
 * engines on one device with equal n_samples and dim_embeddings, at most 128 signatures in total);
 * the result is written to every engine's sample embeddings. */
int salnmf_corr_update_sample_embeddings_multi(salnmf_engine* const* engines, int n_engines,
                                               double variance, int maxiter, int* status_out);
/* CorrNMFDet.update_signature_embeddings (corrnmf_det.py:88-113): one Newton-CG solve per signature
 * (same objective with the roles of signatures and samples exchanged; every evaluation is a pass
 * over all samples, one workgroup per signature).  maxiter <= 0 selects SciPy's default, which is
 * what the reference uses here; status_out has n_signatures ints or is NULL. */
int salnmf_corr_update_signature_embeddings(salnmf_engine* e, double variance, int maxiter,
                                            int* status_out);
/* From 2 048 samples on, the signature solves run in LOCKSTEP (csrc/salnmf_corr_lockstep.h): one evaluation round
 * per launch over (chunks x signatures) workgroups, the K Newton-CG solvers replayed from their evaluation logs
 * between rounds -- 3x faster than one workgroup per signature at c5, and shardable: a sample-sharded engine
 * all-reduces the 66 + dim^2 sums per signature of every round (through the peer exchange where they fit its inbox).  0 forces the single-kernel form; the two agree
 * to rounding of the sums. */
int salnmf_set_lockstep(salnmf_engine* e, int on);
/* The sample solves (both entry points above) run BATCHED where the shape allows (at most 80 signatures over all
 * modalities, dim_embeddings <= 48; csrc/salnmf_corr_batched.hip): sixteen solves per wavefront advance in lockstep
 * rounds, every round's evaluations as two fp64 MFMA products with the signature embeddings, the solver being the
 * resumable form of the same Newton-CG (csrc/salnmf_ncg_machine.h).  0 forces one wavefront per sample
 * (csrc/salnmf_corr_kernels.h), which larger shapes always use; the two agree to rounding of the sums (same solver,
 * same problems, another summation order). */
int salnmf_set_batched_sample_solves(salnmf_engine* e, int on);

/* Opt-in fast mode of salnmf_kl_step: the joint update_WH step on the fp32 matrix cores (fp32 copies of X and H are made
 * on the device; W, the numerator's cross-workgroup sums and the W tail stay fp64; H is converted back at the end of every
 * salnmf_kl_step call, so every other entry point sees the usual fp64 state).  Unweighted steps only.  Tolerance: W, H
 * within 1e-5 rel-L2 of the fp64 step after 20 steps, within 1e-3 after 500 (the reference computes in fp64,
 * _utils_klnmf.py:7-9; the default SALNMF_PRECISION_F64 is the path all parity claims and benchmarks refer to).
 * Entry by entry, one step lies within (K + V + 8) 2^-24 (H) and 2 (K + 16 T + 8) 2^-24 (W) of the same step computed
 * exactly on the fp32-rounded X, H and W (the tail multiplies the unrounded W); T = tiles of 16 samples per wave,
 * ceil(ntiles / (4 grid)).  An entry below EPSILON comes back as EPSILON exactly; relative, because every sum has
 * non-negative terms (tests/_f32_ref.py). */
#define SALNMF_PRECISION_F64 0
#define SALNMF_PRECISION_F32_FAST 1
int salnmf_set_precision(salnmf_engine* e, int precision);
/* The same solves with the sample-side inputs handed over by the caller: n_all samples (of ALL shards, in
 * global order) with embeddings U_all (n_all x dim), scalings alpha_all (n_all) and aux_all (n_all x
 * n_signatures, compact), host pointers.  This is the exchange point of a sample-sharded CorrNMF update
 * (mmcorrnmf.py:347-396 / corrnmf_det.py:88-113 need sums over all samples): with a communicator attached
 * salnmf_corr_update_signature_embeddings gathers these three arrays itself over RCCL; this entry point lets a
 * host-side collective (any torch.distributed backend) do the gather instead.  Result: the engine's
 * signature embeddings. */
int salnmf_corr_update_signature_embeddings_from(salnmf_engine* e, int64_t n_all, const double* U_all,
                                                 const double* alpha_all, const double* aux_all,
                                                 double variance, int maxiter, int* status_out);
/* out2[0] = sum of squares of the signature embeddings, out2[1] = of the sample embeddings: what
 * update_variance (corrnmf_det.py:60-69) and the prior terms of elbo_corrnmf
 * (_utils_corrnmf.py:93-98) need from the device-resident embeddings. */
int salnmf_corr_embedding_sumsq(salnmf_engine* e, double* out2);
/* poisson_llh, _utils_klnmf.py:98-160 (the data term of elbo_corrnmf, _utils_corrnmf.py:92). */
int salnmf_corr_poisson_llh(salnmf_engine* e, double* out);

/* ---- Initialisation on the device: the deterministic methods of
 * src/salamander/initialization/methods.py on the resident X, so that a default fit does not spend its time in a
 * host SVD.  The host layer (salamander_amd/device_init.py) drives them; the signature side (n_features <= 96)
 * stays on the host.
 *   init_gram:    gram_out (n_features x n_features) = X^T X and xsum_out = sum of all entries of X (both over ALL
 *                 shards when a communicator is attached).  The right singular vectors of X are its eigenvectors:
 *                 what sklearn's _initialize_nmf (methods.py:83) obtains from a randomized SVD.
 *   init_project: H <- X B^T for B (n_signatures x n_features, host), i.e. the left singular vectors for
 *                 B = V^T / sigma; posneg_out[0..K) / [K..2K) = squared norms of the positive / negative parts of
 *                 every column (all shards): all the NNDSVD sign split needs from the left factor.
 *   init_finish:  H <- clip(fill(threshold(scale_j * part_j(H))) * post_j): the chosen sign part (column 0: |.|),
 *                 sklearn's `W[W < eps] = 0`, the "nndsvda" fill (0 = none), the exposure scaling of normalize_WH
 *                 (initialize.py:116) and the EPSILON clip (:117).
 *   init_flat:    methods.py:58-66 + the same post-processing: H[n][j] = clip(rowsum(X_n) / n_signatures * post_j). */
int salnmf_init_gram(salnmf_engine* e, double* gram_out, double* xsum_out);
int salnmf_init_project(salnmf_engine* e, const double* B, double* posneg_out);
int salnmf_init_finish(salnmf_engine* e, const double* scale, const int* take_neg, const double* post,
                       double zero_below, double fill);
int salnmf_init_flat(salnmf_engine* e, const double* post /* n_signatures */);
/* separableNMF (methods.py:112-135), the signature side: n_select rounds of successive projection on the resident X
 * (every sample normalised to sum 1; argmax of the squared norms with np.argmax's tie rule; rank-1 deflation) ->
 * chosen_out[n_select] = the selected sample indices in selection order.  The exposures of that method come from the
 * host's legacy RNG (methods.py:133) and stay with the host layer.  Unsharded engines only.  norms_out receives the winning squared norm of every round: after deflation by a
 * rank-deficient or duplicated selection the remaining norms are at rounding level and the device's argmax (fused
 * multiply-adds, another summation order) may then differ from np.argmax on the host -- the caller compares
 * norms[k] with norms[0] and keeps the host's selection for such inputs (salamander_amd/models/standard_nmf.py). */
int salnmf_init_separable(salnmf_engine* e, int n_select, int64_t* chosen_out, double* norms_out /* n_select or NULL */);

/* Multi-GPU: one engine per process/GPU, sample axis sharded; the only exchange is an
 * RCCL all-reduce of the (K x V) numerator per W update (+ scalars for objectives; CorrNMF adds one gather
 * of the sample-side inputs of the signature-embedding solves per update).
 * Rank 0 obtains an id, the host layer broadcasts it, every rank calls comm_init. */
#define SALNMF_UNIQUE_ID_BYTES 128
int salnmf_comm_unique_id(char* out_id /* SALNMF_UNIQUE_ID_BYTES */);
int salnmf_comm_init(salnmf_engine* e, const char* id, int n_ranks, int rank);
/* Number of ranks, this engine's rank, and the number of samples over all shards (n_samples of this engine
 * when no communicator is attached).  Any output may be NULL. */
int salnmf_comm_info(salnmf_engine* e, int* n_ranks, int* rank, int64_t* n_samples_total);
/* What the exchange layers THEMSELVES report about this engine, as opposed to what the caller passed to comm_init /
 * p2p_connect (the reference has no counterpart: SURVEY.md 8e; a benchmark line that claims N ranks quotes these):
 *   rccl_nranks, rccl_rank, rccl_device : ncclCommCount / ncclCommUserRank / ncclCommCuDevice of the attached
 *       communicator; -1 without a communicator (or if the RCCL in the process lacks the query)
 *   p2p_nranks        : ranks of the connected peer-to-peer exchange (0 when not connected)
 *   p2p_inboxes_mapped: inboxes this engine holds a mapping of, its own included (== p2p_nranks when connected)
 *   peer_devices      : SALNMF_P2P_MAX_RANKS ints, the HIP device (as this process numbers them) on which rank r's inbox
 *       lives, -1 for ranks beyond p2p_nranks or where the runtime cannot tell for an IPC mapping
 *   device, pci_bus_id: this engine's HIP device and its PCI bus id ("0000:05:00.0", SALNMF_PCI_BUS_ID_BYTES incl. NUL)
 * Any output may be NULL. */
#define SALNMF_P2P_MAX_RANKS 8
#define SALNMF_PCI_BUS_ID_BYTES 32
int salnmf_comm_observed(salnmf_engine* e, int* rccl_nranks, int* rccl_rank, int* rccl_device, int* p2p_nranks, int* p2p_inboxes_mapped,
                         int* peer_devices /* SALNMF_P2P_MAX_RANKS */, int* device, char* pci_bus_id /* SALNMF_PCI_BUS_ID_BYTES */);

/* Peer-to-peer exchange for the small all-reduces (the K x V numerator, the MvNMF line-search sums, objective scalars):
 * every rank stores its vector straight into an inbox on each peer of the node (hipIpc-mapped uncached memory, xGMI
 * peer stores) and adds the n vectors in rank order, so all ranks hold bit-identical sums.  It replaces the library
 * all-reduce where that is pure latency (38 KB at K = 50); larger exchanges keep using RCCL.  One node, <= 8 ranks.
 *   export : allocates this engine's inbox for vectors of up to max_count doubles (<= 16384) and returns its IPC handle
 *   connect: maps the peers' inboxes; `handles` = n_ranks * SALNMF_P2P_HANDLE_BYTES in rank order (the host layer
 *            all-gathers them); n_samples_total = samples over all shards (used when no RCCL communicator is attached)
 *   set_p2p: switch the exchange off / on again (off: the all-reduces go through RCCL, which must then be attached)
 *   set_p2p_timeout_ms: how long a rank waits for a peer inside an exchange before it gives up (default 20 000 ms:
 *            the ranks' host threads may be that far apart)
 * Every rank must issue the same sequence of calls on its engine.  A rank that waits 20 s for a peer gives up: the
 * next download / objective call on that engine fails, and its later exchanges return at once.  Destroy the engines only after all ranks are done. */
#define SALNMF_P2P_HANDLE_BYTES 64
int salnmf_p2p_export(salnmf_engine* e, int n_ranks, int64_t max_count, char* handle_out /* SALNMF_P2P_HANDLE_BYTES */);
int salnmf_p2p_connect(salnmf_engine* e, int rank, int n_ranks, const char* handles, int64_t n_samples_total);
int salnmf_set_p2p(salnmf_engine* e, int on);
int salnmf_set_p2p_timeout_ms(salnmf_engine* e, int64_t timeout_ms);

/* The joint step split at the exchange point, for a caller-side collective
 * (e.g. torch.distributed on a wrapped device pointer):
 *   partial: fused pass + local reduction -> SALNMF_BUF_G, H updated in place
 *   finish : W tail from SALNMF_BUF_G (after the caller's all-reduce) */
int salnmf_kl_step_partial(salnmf_engine* e);
int salnmf_kl_step_finish(salnmf_engine* e, int n_given, int clip_mode);
/* Device address of one of the engine's buffers (SALNMF_BUF_*).  Query it when needed instead of caching it:
 * an MvNMF step exchanges the W buffer with its trial buffer rather than copying. */
void* salnmf_device_ptr(salnmf_engine* e, int which);
void* salnmf_stream(salnmf_engine* e);
int salnmf_sync(salnmf_engine* e);

/* Measurement: run n_steps joint steps on the engine's stream; every sample_stride-th step carries HIP events bound
 * to its two dispatches (start / stop of the fused update kernel and of the W tail: the kernels' own durations, the
 * figure rocprofv3 reports -- events recorded around a launch would add their barrier packets to it).  Outputs (any may
 * be NULL): total ms over the n_steps (events recorded before the first and after the last launch), and the average
 * duration in ms of the fused update kernel and of the W tail over the samples. */
int salnmf_profile_kl_steps(salnmf_engine* e, int n_steps, int n_given, int sample_stride,
                            double* total_ms, double* fused_avg_ms, double* tail_avg_ms);
/* Same for the forward (W@H) + objective kernel: average duration over n_calls. */
/* Where a SHARDED joint step's microseconds go, on this rank: n_steps steps with HIP events bound to the two dispatches of
 * every step and s_memrealtime stamps inside the tail's exchange (csrc/salnmf_p2p_kernels.h: tail_p2p_kernel).  out9, in
 * microseconds: [0] step (stream time / n_steps) [1] fused pass [2] tail + exchange launch; per row workgroup of the tail,
 * averaged over rows and steps: [3] local slab reduction [4] stores to the peers [5] wait for the peers' rows (the payload
 * carries its arrival tag: salnmf_p2p_kernels.h) [6] sum of the rows [7] W row finish; [8] the longest such wait of any row
 * and step.  Needs the
 * peer-to-peer exchange (a one-rank world included); every rank of the world must call it with the same n_steps. */
int salnmf_profile_sharded_steps(salnmf_engine* e, int n_steps, int n_given, double* out9);
int salnmf_profile_objective(salnmf_engine* e, int n_calls, double* avg_ms);
/* Same for the forward kernel alone (H @ W written to a scratch buffer, no objective terms). */
int salnmf_profile_reconstruct(salnmf_engine* e, int n_calls, double* avg_ms);

/* ---- Batched sweeps (KLNMFSweep, salamander_amd/models/sweep.py): many independent KLNMF models -- different
 * n_signatures, different initialisations -- on ONE count matrix or on bootstrap resamples of it (below), one workgroup per model, every model's step, objective
 * and per-sample divergences in one launch for all of them.  What the reference's tutorial does one fit after another to
 * choose the number of signatures (tutorial.ipynb section 1.6: KLNMF(n_signatures=k).fit(adata.copy()) for k = 1..9).
 * Limits: n_features <= 96, n_samples <= 1024 (64 tiles of 16), 1 <= n_signatures <= 16 per member, unweighted.  Every
 * member's W, H and objectives are bit for bit what an engine of that shape computes (salnmf_kl_step,
 * salnmf_objective_async, salnmf_samplewise_kl): the step and the passes call the same bodies as the small-cohort kernel
 * and the forward kernel, with the engine's grid (csrc/salnmf_batch.h).  Errors of these entry points:
 * salnmf_batch_last_error. */
typedef struct salnmf_batch salnmf_batch;
#define SALNMF_BATCH_SLOTS 256 /* rows of the objective array: one row per convergence test, one column per member */
const char* salnmf_batch_last_error(void);
/* n_signatures: n_members values.  Members are numbered 0 .. n_members - 1 in that order. */
int salnmf_batch_create(int device, int n_features, int64_t n_samples, int n_members, const int* n_signatures,
                        salnmf_batch** out);
void salnmf_batch_destroy(salnmf_batch* b);
/* The count matrix (n_samples x n_features) shared by all members; clip != 0: X.clip(EPSILON) on the way, as
 * SignatureNMF._setup_adata does (signature_nmf.py:281). */
int salnmf_batch_upload_X(salnmf_batch* b, const double* X, int clip);
/* One member's initial W (n_signatures x n_features) and H (n_samples x n_signatures), as salnmf_upload_W / _H. */
int salnmf_batch_upload_member(salnmf_batch* b, int member, const double* W, const double* H);
int salnmf_batch_download_member(salnmf_batch* b, int member, double* W, double* H);
/* n_steps joint updates (update_WH, _utils_klnmf.py:281-361) of each listed member, n_given[i] of member members[i]'s
 * first signatures kept (0 <= n_given[i] < its n_signatures); one launch of n_active workgroups per 4 096 steps.  Members
 * not listed are left as they are. */
int salnmf_batch_kl_step(salnmf_batch* b, int n_steps, int n_active, const int* members, const int* n_given);
/* Per-sample weights of one member, as salnmf_set_weights gives them to an engine: weights_kl scales every sample's KL
 * term, weights_lhalf is its l-half penalty weight (with it the step takes the penalised closed form of the exposure
 * update, also where every entry is 0).  Each argument is n_samples doubles or NULL; NULL / NULL clears the member's
 * weights.  Negative or non-finite entries are refused before anything is copied.  A weighted member's steps and queued
 * objectives are, bit for bit, those of an engine with the same weights; salnmf_batch_samplewise_kl and _heldout_kl stay
 * unweighted.  One salnmf_batch_kl_step call may list weighted and unweighted members together (two launches then). */
int salnmf_batch_set_weights(salnmf_batch* b, int member, const double* weights_kl, const double* weights_lhalf);
/* KLNMF.objective_function (klnmf.py:64-80, kl_divergence _utils_klnmf.py:11-55) of each listed member into row `slot` of
 * the objective array (pinned host memory, written by the reducing workgroup), no host round trip.  Entries of members not
 * listed keep what they held. */
int salnmf_batch_objective_async(salnmf_batch* b, int slot, int n_active, const int* members);
/* Rows [first, first + count) of the objective array -> out (count x n_members): waits for those rows only. */
int salnmf_batch_objective_read(salnmf_batch* b, int first, int count, double* out);
/* samplewise_kl_divergence (_utils_klnmf.py:58-97) of every member -> out (n_members x n_samples). */
int salnmf_batch_samplewise_kl(salnmf_batch* b, double* out);

/* ---- Bootstrap resamples of a count matrix, drawn on the device (csrc/salnmf_resample.h).  X (n_samples x n_features) holds
 * non-negative integer values with row totals T_n < 2^32.  Row n of resample r is one multinomial draw of T_n trials with
 * probabilities X[n, :] / T_n, built as T_n categorical draws:
 *   generator: Philox4x32-10 (Salmon et al., Random123), key = (seed & 0xffffffff, seed >> 32);
 *   block q of row n of resample r: counter (q mod 2^32, q >> 32, n, r) -> words (o0, o1, o2, o3);
 *   draw 2q uses u = o0 | o1 << 32, draw 2q + 1 uses u = o2 | o3 << 32; draws j >= T_n are discarded;
 *   t = floor(u T_n / 2^64); the draw lands in the smallest v with cum[v] > t, cum[v] = sum_{w <= v} X[n, w].
 * Integer arithmetic throughout: the same bits on every run, row totals kept, zero cells stay zero, and resample r does not
 * depend on n_resamples.  The bias of a draw against the exact probabilities is at most T_n / 2^64.  Both entry points
 * refuse, before any launch, a negative or non-integer entry and a row total >= 2^32 (status 1, salnmf_last_error names the
 * row); 1 <= n_resamples <= 65535. */
/* Stand-alone: upload, draw, download.  n_features <= 3072.  out: n_resamples x n_samples x n_features, plain counts. */
int salnmf_resample_counts(int device, const double* X, int64_t n_samples, int n_features, int n_resamples, uint64_t seed,
                           double* out);
/* n_resamples resamples of the batch's uploaded X (salnmf_batch_upload_X first), drawn device to device into slots in X's
 * own layout -- pad rows and columns 0, entries max(count, SALNMF_EPSILON) as upload_X(clip = 1) leaves them -- each with its
 * x log x constants.  "Dataset" r is slot r, dataset -1 the uploaded X.  A second call, or another upload of X, drops the
 * slots and puts every member back on dataset -1. */
int salnmf_batch_resample(salnmf_batch* b, int n_resamples, uint64_t seed);
/* The dataset a member's steps, objectives and per-sample divergences read from now on (-1 at creation). */
int salnmf_batch_set_dataset(salnmf_batch* b, int member, int dataset);
/* raw == 0: the dataset as n_samples x n_features; a resample comes back as plain counts (the clipped zeros restored to 0),
 * dataset -1 as the device holds it.  raw != 0: the slot as the kernels read it, 16 ceil(n_samples / 16) x 96. */
int salnmf_batch_download_dataset(salnmf_batch* b, int dataset, int raw, double* out);
/* Development aid (tools/bench_bootstrap.py): salnmf_batch_resample once, then n_calls launches of the resample kernel
 * alone between two events -> average milliseconds per launch.  The slots hold the same resamples afterwards. */
int salnmf_profile_resample(salnmf_batch* b, int n_resamples, uint64_t seed, int n_calls, double* avg_ms);

/* ---- Count splitting (Poisson thinning) of a count matrix, drawn on the device (csrc/salnmf_split.h).
 * X as for the resampler: non-negative integer values, row totals T_n < 2^32.  Every single mutation goes to the training
 * matrix with probability thr / 2^64, independently; for Poisson counts the two halves are independent Poisson counts:
 *   thr = (uint64) floor(train_fraction * 2^64), 1 <= thr <= 2^64 - 1 (the fraction itself never crosses this boundary);
 *   mutation j of row n (0 <= j < T_n) belongs to cell v(j), the smallest v with cum[v] > j, cum[v] = sum_{w <= v} X[n, w];
 *   generator: Philox4x32-10, key = (seed & 0xffffffff, seed >> 32);
 *   block q of row n of split f: counter (q, 0x53504C54, n, f) -> words (o0, o1, o2, o3) -- the resampler's second counter
 *   word is always 0, so the two streams never meet under one seed;
 *   draw 2q uses u = o0 | o1 << 32, draw 2q + 1 uses u = o2 | o3 << 32; draws j >= T_n are discarded;
 *   mutation j goes to train iff u_j < thr.
 * train_f[n, v] counts the mutations of cell v sent to train, test_f[n, v] = X[n, v] - train_f[n, v].  Integer arithmetic
 * throughout: the same bits on every run, zero cells stay zero in both halves, split f does not depend on n_splits.  The
 * entry points refuse, before any launch, what the resampler refuses, thr == 0 and n_splits outside [1, 32767]. */
/* Stand-alone: upload, draw, download.  n_features <= 3072.  train_out, test_out: n_splits x n_samples x n_features each,
 * plain counts. */
int salnmf_split_counts(int device, const double* X, int64_t n_samples, int n_features, int n_splits, uint64_t thr, uint64_t seed,
                        double* train_out, double* test_out);
/* n_splits splits of the batch's uploaded X (salnmf_batch_upload_X first) into 2 n_splits slots in X's own layout -- pad rows
 * and columns 0, entries max(count, SALNMF_EPSILON) -- each with its x log x constants: train split f is dataset f, test
 * split f dataset n_splits + f, for salnmf_batch_set_dataset, _download_dataset and _heldout_kl.  A second call, or another
 * upload of X, drops the slots and puts every member back on dataset -1.  Splits and resamples exclude each other on one
 * batch: with resamples drawn this call is refused, and salnmf_batch_resample is refused once a split is drawn (upload X
 * again to drop either). */
int salnmf_batch_split(salnmf_batch* b, int n_splits, uint64_t thr, uint64_t seed);
/* Held-out scoring: samplewise_kl_divergence of member members[i] against dataset datasets[i] instead of its own, with its
 * exposures read as max(scale * H, EPSILON) -> out (n_members x n_samples).  The forward pass's per-sample mode, unchanged,
 * on the engine's grid for the shape: the bits an engine holding that dataset, the member's W and the scaled, clipped H
 * computes (salnmf_samplewise_kl).  For a member fitted on train split f, dataset n_splits + f and
 * scale = (1 - train_fraction) / train_fraction give the out-of-sample Poisson deviance.  The members' own state, datasets
 * included, is left as it is.  members: each at most once; scale positive and finite. */
int salnmf_batch_heldout_kl(salnmf_batch* b, int n_members, const int* members, const int* datasets, double scale, double* out);
/* Development aid (tools/bench_split.py): salnmf_batch_split once, then n_calls launches of the split kernel alone between
 * two events -> average milliseconds per launch.  The slots hold the same splits afterwards. */
int salnmf_profile_split(salnmf_batch* b, int n_splits, uint64_t thr, uint64_t seed, int n_calls, double* avg_ms);

/* ---- Signature stability: match, cluster and score the signatures of many fits (csrc/salnmf_stability.h, DESIGN.md
 * section 12 "Stability").  A group is M >= 2 signature matrices of one shape K x V (K <= 16, V <= 96) and one error value
 * per member (errors == NULL: all zero).  Per group: rows are scaled to unit Euclidean norm; the member of smallest error
 * (lowest index on ties) provides the first centroids; each round assigns every member's rows to the centroids by the
 * optimal assignment under the cost 1 - cosine, sums the rows of each cluster over the members in ascending order, and stops
 * when no assignment changed (the first round always counts as changed) or after max_rounds rounds; otherwise the normalised
 * sums are the next centroids.  Silhouettes under the cosine distance follow from the cluster sums.
 * One launch handles all groups.  With T the number of listed members over all groups, in group order, and G = n_groups,
 * the outputs are padded to 16 signatures and 96 features:
 *   assignments  T x 16 (row of the member assigned to cluster j; entries j >= K hold j)
 *   a, b, silhouette  T x 16 (point j of a member is its row assigned to cluster j: mean distance to its own cluster without
 *                itself, smallest mean distance to another cluster, (b - a) / max(a, b); for K = 1, b is NaN and the
 *                silhouette 1; entries j >= K are 0)
 *   n_rounds, converged  G;  consensus  G x 16 x 96 (cluster sums scaled to row sum 1);  cluster_stability  G x 16 (mean
 *                silhouette of a cluster over the members);  stability  G x 2 (mean and minimum of cluster_stability)
 *   kernel_ms    NULL, or one double: the launch's milliseconds by device events.
 * Arguments are validated before any launch (a NaN among the errors is refused too); errors: salnmf_batch_last_error. */
/* In place: group g lists members[group_offsets[g] .. group_offsets[g + 1]) of the batch (group_offsets: n_groups + 1 values
 * from 0), all of one n_signatures; the kernel reads the members' W where the steps left it.  errors: one per listed member. */
int salnmf_batch_stability(salnmf_batch* b, int n_groups, const int* group_offsets, const int* members, const double* errors,
                           int max_rounds, int* assignments, int* n_rounds, int* converged, double* consensus, double* a,
                           double* b_dist, double* silhouette, double* cluster_stability, double* stability, double* kernel_ms);
/* Stand-alone: signatures is T x 16 x 96, zero padded, group after group (n_members[g] matrices of n_signatures[g] rows
 * and n_features columns each).  Also refused: a row that is not finite or has norm zero. */
int salnmf_signature_stability(int device, const double* signatures, int n_groups, const int* n_signatures,
                               const int* n_members, int n_features, const double* errors, int max_rounds, int* assignments,
                               int* n_rounds, int* converged, double* consensus, double* a, double* b_dist, double* silhouette,
                               double* cluster_stability, double* stability, double* kernel_ms);

/* ---- Refit of exposures to FIXED signatures, with bootstrap intervals (csrc/salnmf_refit.h).
 * counts is n_samples x n_features (n_features <= 96), signatures n_signatures x n_features (n_signatures <= 96), used as
 * they are (never clipped; the caller scales the rows to sum 1).  Every (sample, dataset) pair is a problem of its own,
 * dataset -1 the counts and dataset r resample r of salnmf_resample_counts(counts, n_resamples, seed), drawn device to
 * device in chunks whose buffer stays within chunk_bytes (<= 0: 256 MiB; at least one resample per chunk; the results do not
 * depend on it):
 *   x = max(row, SALNMF_EPSILON);  h_k = (sum_v x_v) / n_signatures;
 *   step (update_H, _utils_klnmf.py:258-264): wh = h W, a = x / wh, h_k <- max(h_k sum_v W[k, v] a_v, SALNMF_EPSILON);
 *   objective: the row's KL divergence as salnmf_samplewise_kl defines it, at iteration 0 and every multiple of
 *   conv_test_freq; the problem stops at the first test at or after min_iterations with |prev - cur| / |prev| < tol (false
 *   for a NaN), converged, else at max_iterations.  A problem's result depends on its own row and the signatures only.
 * Outputs: exposures n_samples x n_signatures; errors (the objective where the problem stopped), n_iterations, converged
 * n_samples.  With n_resamples R > 0 (R <= 1024: the reduction sorts a signature's R values in one pass):
 *   n_iterations_resampled, errors_resampled  R x n_samples;  exposures_resampled  NULL, or R x n_samples x n_signatures;
 *   exposures_mean  n_samples x n_signatures: the sum over r in ascending order, divided by R;
 *   exposures_quantiles  n_quantiles x n_samples x n_signatures (n_quantiles <= 16): of the R sorted values the one at index
 *   floor(q (R - 1)) for q <= 0.5 and ceil(q (R - 1)) for q > 0.5.
 * With R > 0 the counts must be what salnmf_resample_counts accepts.  timings: NULL, or 4 doubles -- milliseconds by device
 * events of the resample launches, the refit launches and the reduction, and the number of chunks.
 * Everything is validated on the host before any launch; status 1 and salnmf_last_error otherwise. */
int salnmf_refit_exposures(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                           int n_signatures, int n_resamples, uint64_t seed, int n_quantiles, const double* quantiles,
                           int min_iterations, int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes,
                           double* exposures, double* errors, int* n_iterations, int* converged, double* exposures_quantiles,
                           double* exposures_mean, int* n_iterations_resampled, double* errors_resampled,
                           double* exposures_resampled, double* timings);

/* ---- Sparse assignment: which of the fixed signatures are active in each sample (csrc/salnmf_assign.h, DESIGN.md
 * section 14).  Arguments, problems, resamples and chunking as salnmf_refit_exposures, plus max_kl_increase (finite) and the
 * requirement max_iterations % conv_test_freq == 0 (the solves of a problem follow one another inside one wave, whose tests
 * stay on common iterations).  Contract, per problem:
 *   a SOLVE from a start h with an active set A is the refit's iteration on the active entries -- the same step, objective and
 *   stop rule, iterations counted from 0 at the start of the solve, the objective evaluated at iteration 0 and at every
 *   multiple of conv_test_freq; inactive entries are exactly 0.0 and stay 0.0 (never clipped up to SALNMF_EPSILON);
 *   phase 0: A = all signatures, h_k = (sum_v x_v) / n_signatures, solve: bit for bit salnmf_refit_exposures' exposures, error,
 *   iteration count and convergence flag (the dense_* outputs);
 *   rounds: the candidate c is the active, not yet protected signature of smallest h, lowest index on equal values; the
 *   procedure stops when there is none or one signature is left.  Trial: copy h, set entry c to 0.0, solve with A \ {c}:
 *   h', f'.  If f' - f <= max_kl_increase (false for a NaN) A, h, f become the trial's; otherwise c is protected for the rest
 *   of the procedure and h, f stay.  Every signature is tried at most once.
 * Outputs: exposures n_samples x n_signatures (0.0 off the support); active (1 / 0), removal_round (the 0-based number of the
 * trial that removed k, -1 if kept), kl_increase (f' - f of the trial that tested k, NaN if never tested) n_samples x
 * n_signatures; errors (f), n_trials, n_iterations (summed over the solves), converged (every solve stopped on its
 * tolerance) n_samples.  With n_resamples R > 0 the whole procedure runs for every resample, and the R exposures are reduced
 * on the device: selection_frequency n_samples x n_signatures = (resamples with exposure > 0) / R, counted in integers;
 * exposures_mean and exposures_quantiles by salnmf_refit_exposures' rules, zeros included; exposures_resampled NULL, or R x
 * n_samples x n_signatures.  timings: NULL, or 4 doubles -- milliseconds by device events of the resample launches, the
 * assignment launches and the reductions, and the number of chunks.
 * Everything is validated on the host before any launch; status 1 and salnmf_last_error otherwise. */
int salnmf_assign_signatures(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                             int n_signatures, int n_resamples, uint64_t seed, int n_quantiles, const double* quantiles,
                             int min_iterations, int max_iterations, int conv_test_freq, double tol, double max_kl_increase,
                             int64_t chunk_bytes, double* exposures, int* active, double* errors, int* removal_round,
                             double* kl_increase, int* n_trials, int64_t* n_iterations, int* converged, double* dense_exposures,
                             double* dense_errors, int* dense_n_iterations, int* dense_converged, double* selection_frequency,
                             double* exposures_quantiles, double* exposures_mean, double* exposures_resampled, double* timings);

/* salnmf_assign_signatures with candidate sets, required signatures and a re-addition pass.
 * salnmf_assign_signatures is this call with candidates = NULL, required = NULL, readd = 0, and keeps its bits.
 *   candidates  NULL (every signature), or n_samples x n_signatures bytes, nonzero = signature k is a candidate in sample n:
 *               the set C_n, which must not be empty;
 *   required    NULL (none), or n_samples x n_signatures bytes: the set R_n, a subset of C_n;
 *   readd       0 or 1.
 * The sets of sample n hold for its counts and for every resample of them.  Contract, per problem:
 *   phase 0: A = C_n, h_k = (sum_v x_v) / |C_n| for k in C_n and exactly 0.0 elsewhere, solve (the dense_* outputs; with every
 *   signature a candidate this is salnmf_assign_signatures' phase 0 bit for bit);
 *   backward rounds as above, with the protected set starting as R_n: a required signature is never a candidate for removal,
 *   its kl_increase stays NaN and its removal_round -1; the rounds stop when there is no candidate or one signature is left;
 *   re-addition pass (readd = 1), after the rounds have ended with (A, h, f): the pool is C_n \ A, each member tried at most
 *   once.  At the accepted h every pool member has the update factor u_k = sum_v W[k, v] x_v / (h W)_v, the step's own factor;
 *   u_k <= 1 is the KKT condition of a zero entry.  The candidate c is the untried pool member of largest u_k (strictly
 *   larger than every one before it in ascending k, so the lowest index wins on equal values and a NaN never wins).  If there
 *   is none, or not u_c > 1, the procedure ends.  Trial: copy h, set entry c to (sum_v x_v) / |C_n|, solve with A + {c}: h', f'.
 *   If f - f' > max_kl_increase (false for a NaN) A, h, f become the trial's, otherwise they stay; either way c is tried.  There
 *   is no second backward pass, so a problem sees at most (n_signatures - 1) + n_signatures trials.
 * Further outputs, n_samples x n_signatures, both may be NULL when readd is 0 and are not written then: readd_round (the
 * 0-based number, continuing the backward count, of the trial that re-added k, -1 otherwise) and kl_decrease (f - f' of the
 * re-addition trial of k, NaN if never tried).  n_trials, n_iterations and converged cover both passes; removal_round keeps the
 * round that removed k even where k is re-added: active and exposures tell the final state.
 * Validated on the host before any launch, with everything else: a sample without a candidate, a required signature that is
 * not a candidate, readd other than 0 or 1. */
int salnmf_assign_signatures_ex(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                                int n_signatures, int n_resamples, uint64_t seed, int n_quantiles, const double* quantiles,
                                int min_iterations, int max_iterations, int conv_test_freq, double tol, double max_kl_increase,
                                int64_t chunk_bytes, const uint8_t* candidates, const uint8_t* required, int readd,
                                double* exposures, int* active, double* errors, int* removal_round, double* kl_increase,
                                int* n_trials, int64_t* n_iterations, int* converged, double* dense_exposures,
                                double* dense_errors, int* dense_n_iterations, int* dense_converged, double* selection_frequency,
                                double* exposures_quantiles, double* exposures_mean, double* exposures_resampled,
                                int* readd_round, double* kl_decrease, double* timings);

/* ---- Goodness of fit of a sample to a catalogue by parametric bootstrap (csrc/salnmf_gof.h).
 * A model draw: row n of draw b is one multinomial draw of totals[n] trials from the spectrum of exposures h = exposures[n, :]
 * under the signatures W (rows of sum one; n_signatures <= 96, n_features <= 96):
 *   P_v = sum_k h_k W[k, v], from 0.0 in ascending k, every term a rounded product followed by a rounded sum (no fused
 *   multiply-add);  S = sum_v P_v, from 0.0 in ascending v.  With S == 0, S not finite or totals[n] == 0 the row is zero;
 *   m_v = (uint64) floor((P_v / S) 2^40) (IEEE division, truncating conversion), cum_v their 64-bit prefix sums, M = cum_{V-1};
 *   generator: Philox4x32-10, key = (seed & 0xffffffff, seed >> 32);
 *   block q of row n of draw b: counter (q, 0x474F4644, n, b) -> words (o0, o1, o2, o3) -- the resampler's second counter word
 *   is 0 and the split's 0x53504C54, so the three streams never meet under one seed;
 *   draw 2q uses u = o0 | o1 << 32, draw 2q + 1 uses u = o2 | o3 << 32; draws j >= totals[n] are discarded;
 *   t = floor(u M / 2^64), and the draw lands in the smallest v with cum_v > t.
 * Integer arithmetic after the weights: the same bits on every run, cells of weight 0 stay 0, draw b does not depend on
 * n_draws.  Refused before any launch: exposures or signatures that are not finite or are negative, totals that are not
 * integers in [0, 2^32), n_draws outside [1, 65536].  out: n_draws x n_samples x n_features, plain counts. */
int salnmf_draw_model_counts(int device, const double* exposures, int64_t n_samples, int n_signatures, const double* signatures,
                             int n_features, const double* totals, int n_draws, uint64_t seed, double* out);
/* The test: the observed counts are refitted exactly as salnmf_refit_exposures refits them (exposures, errors, n_iterations,
 * converged: the same bits); draw b is salnmf_draw_model_counts of those exposures -- read where the refit left them on the
 * device -- with the rows' own totals, written device to device as max(count, SALNMF_EPSILON) in chunks whose buffer stays
 * within chunk_bytes (<= 0: 256 MiB; at least one draw per chunk; the results do not depend on it), and refitted in the same
 * way: null_errors and null_n_iterations, n_draws x n_samples, are bit for bit what salnmf_refit_exposures returns for the
 * draw.  Reduction, one thread per sample in ascending b: n_exceed[n] counts the draws with null_errors[b, n] >= errors[n]
 * (false for a NaN on either side); null_mean[n] is the sum of null_errors[b, n] from 0.0, divided by n_draws.  The p-value is
 * (1 + n_exceed) / (n_draws + 1).  draws: NULL, or n_draws x n_samples x n_features, plain counts.  The counts must be what
 * salnmf_resample_counts accepts, n_draws in [1, 65536].  timings: NULL, or 4 doubles -- milliseconds by device events of the
 * draw launches, the refit launches and the reduction, and the number of chunks.
 * Everything is validated on the host before any launch; status 1 and salnmf_last_error otherwise. */
int salnmf_goodness_of_fit(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                           int n_signatures, int n_draws, uint64_t seed, int min_iterations, int max_iterations, int conv_test_freq,
                           double tol, int64_t chunk_bytes, double* exposures, double* errors, int* n_iterations, int* converged,
                           int* n_exceed, double* null_mean, double* null_errors, int* null_n_iterations, double* draws,
                           double* timings);

/* ---- Is signature s present in this sample?  A nested pair of fits against its own parametric-bootstrap null
 * (csrc/salnmf_presence.h).  counts, signatures, the iteration arguments and chunk_bytes as
 * salnmf_goodness_of_fit, plus max_iterations % conv_test_freq == 0 as salnmf_assign_signatures; test: n_test distinct signature
 * indices in [0, n_signatures); candidates: NULL (every signature), or n_samples x n_signatures bytes as
 * salnmf_assign_signatures_ex takes them (the set C_n, not empty).  Contract, for sample n and s = test[j]:
 *   a SOLVE ON A SET A is salnmf_assign_signatures_ex's phase 0 with candidates = A: h_k = (sum_v x_v) / |A| on A and exactly 0.0
 *   off it, the refit's step, objective and stop rule -- bit for bit the exposures, error, iteration count and convergence flag
 *   of that call with candidates = required = A;
 *   the alternative is the solve on C_n (h1, f1), the null the solve on C_n \ {s} (h0, f0); statistic[n, j] = f0 - f1, half the
 *   likelihood-ratio statistic;
 *   the pair is UNTESTED if s is not in C_n or C_n = {s}: tested[n, j] = 0, it draws nothing and costs no solve;
 *   null draw b of the pair is one model draw (above, steps as salnmf_draw_model_counts) of sum_v counts[n, v] trials from the
 *   exposures h0, with the Philox counter (q, 0x50530000 + s, n, b): the second word carries a stream family ("PS" in its upper
 *   half) that no other draw uses -- the resampler's word is 0, the split's 0x53504C54, the goodness-of-fit draw's 0x474F4644 --
 *   and the tested signature, so the draws of a pair depend on (seed, n, s, b) and on h0 only, not on n_samples, n_test,
 *   n_draws, the chunks or what else is tested;
 *   every draw goes through the same two solves from cold starts: null_statistics[b, n, j] = t_b;
 *   reduction, one thread per pair in ascending b: n_exceed[n, j] counts t_b >= statistic[n, j] (false for a NaN on either
 *   side), null_mean[n, j] is the sum of t_b from 0.0, divided by n_draws.  The p-value is (1 + n_exceed) / (n_draws + 1).
 * Outputs: tested (1 / 0), statistic, n_exceed, null_mean, null_errors (f0)  n_samples x n_test;  null_exposures (h0)  n_samples x
 * n_test x n_signatures;  exposures (h1)  n_samples x n_signatures and errors (f1)  n_samples -- every tested pair of a sample
 * solves the same alternative; n_iterations, converged  n_samples x n_test x 2 (alternative, null);  null_statistics  n_draws x
 * n_samples x n_test;  null_n_iterations  n_draws x n_samples x n_test x 2;  draws  NULL, or n_draws x n_samples x n_test x n_features,
 * plain counts.  Entries of an untested pair: NaN in the doubles (0 in draws), 0 in the integers; a sample without a tested pair
 * has NaN exposures and error.  timings: NULL, or 4 doubles -- milliseconds by device events of the draw launches, the solve
 * launches and the reduction, and the number of chunks.
 * Everything is validated on the host before any launch; status 1 and salnmf_last_error otherwise. */
int salnmf_signature_presence(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                              int n_signatures, const int* test, int n_test, const uint8_t* candidates, int n_draws, uint64_t seed,
                              int min_iterations, int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes,
                              uint8_t* tested, double* statistic, int* n_exceed, double* null_mean, double* exposures, double* errors,
                              double* null_exposures, double* null_errors, int* n_iterations, int* converged,
                              double* null_statistics, int* null_n_iterations, double* draws, double* timings);

/* ---- Could the presence test have seen signature s in this sample?  Detection power per (sample, tested signature, share)
 * (csrc/salnmf_power.h).  The arguments of salnmf_signature_presence, then shares: n_shares doubles in
 * [0, 1), strictly ascending; n_alt_draws (A) draws per share; max_exceed: a draw is detected with at most this many null
 * statistics at or above its own -- for a level alpha the largest m >= 0 with (1 + m) / (n_draws + 1) <= alpha, so that
 * "detected" is "the presence test would have given p <= alpha against this null".  Contract, for sample n, s = test[j], share
 * pi_l = shares[l] and alternative draw a:
 *   the presence test runs first, unchanged: its launches, and its outputs bit for bit those of salnmf_signature_presence with
 *   the same arguments; untested pairs stay untested here (NaN in the doubles below, 0 in the integers and the draws, no cost);
 *   planted_exposures[l, n, j, :]: with h0 the pair's null fit where the observed launch left it on the device, S0 = sum_k h0[k]
 *   from 0.0 in ascending k over all n_signatures, c_l = 1.0 - pi_l (one rounded subtraction): Hp[k] = c_l h0[k] for k != s and
 *   Hp[s] = pi_l S0, each one rounded product, no fused multiply-add.  h0[s] is exactly 0, so pi = 0 gives h0 back bit for bit;
 *   alternative draw a of (pair, l) is one model draw (salnmf_draw_model_counts' steps) of sum_v counts[n, v] trials from that
 *   planted row, with the Philox counter (q, 0x50570000 + s, n, a): a stream family of its own ("PW" in the upper half of the
 *   second word).  The level is not in the counter -- all levels of a pair share their random numbers -- so the draw depends on
 *   (seed, n, s, a) and on its planted row and on nothing else: not n_samples, n_test, n_shares, n_alt_draws, n_draws, the
 *   chunks or the other shares;
 *   every draw goes through the presence test's two solves from cold starts: alt_statistics[l, a, n, j] = t*_a and
 *   alt_n_iterations[l, a, n, j, 2], in chunks of rows r = l A + a whose buffer stays within chunk_bytes;
 *   reduction, one thread per (pair, share), everything in ascending order: alt_n_exceed[l, a, n, j] counts the pair's n_draws
 *   null statistics t_b >= t*_a (false for a NaN on either side); draw a is detected iff t*_a is not NaN and that count is
 *   <= max_exceed; n_detected[l, n, j] counts the detected draws; alt_mean[l, n, j] is the sum of t*_a from 0.0 in ascending a,
 *   divided by A.  Power is n_detected / A.
 * The critical value is that of the null drawn from the OBSERVED sample's h0, not re-estimated per alternative draw (that
 * would be a nested bootstrap of A n_draws draws): power at pi = 0 measures this approximation and should sit near alpha.  The
 * planted signature displaces the fitted background proportionally; everything is conditional on the sample's total.
 * Outputs: those of salnmf_signature_presence, then planted_exposures  n_shares x n_samples x n_test x n_signatures;
 * alt_statistics, alt_n_exceed  n_shares x A x n_samples x n_test;  alt_n_iterations  the same x 2;  n_detected, alt_mean
 * n_shares x n_samples x n_test;  alt_draws  NULL, or n_shares x A x n_samples x n_test x n_features, plain counts.  timings: NULL,
 * or 9 doubles -- the presence test's four, then milliseconds by device events of the planting, the alternative draw launches,
 * the alternative solve launches and the power reduction, and the number of chunks of alternative draws.
 * Refused on the host before any launch, status 1 and salnmf_last_error: everything salnmf_signature_presence refuses; n_shares
 * outside [1, 64]; a share that is not finite, is < 0 or >= 1, or is not strictly above its predecessor; n_alt_draws outside
 * [1, 65536]; max_exceed outside [0, n_draws]. */
int salnmf_signature_power(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                           int n_signatures, const int* test, int n_test, const uint8_t* candidates, int n_draws, uint64_t seed,
                           int min_iterations, int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes,
                           const double* shares, int n_shares, int n_alt_draws, int max_exceed,
                           uint8_t* tested, double* statistic, int* n_exceed, double* null_mean, double* exposures, double* errors,
                           double* null_exposures, double* null_errors, int* n_iterations, int* converged,
                           double* null_statistics, int* null_n_iterations, double* draws,
                           double* planted_exposures, double* alt_statistics, int* alt_n_iterations, int* alt_n_exceed,
                           int* n_detected, double* alt_mean, double* alt_draws, double* timings);

/* ---- How far can one exposure move before the sample's fit degrades?  The profile likelihood of h_s per (sample, tested
 * signature), and the confidence interval it gives (csrc/salnmf_profile.h).  counts, signatures, test,
 * candidates, the iteration arguments and max_iterations % conv_test_freq == 0 as salnmf_signature_presence, except that the
 * counts need not be integers: nothing is drawn.  Contract, for sample n with set C_n, s = test[j] and a value c >= 0:
 *   the pair is tested or UNTESTED by salnmf_signature_presence's rule, and its alternative fit (h1, f1: exposures, errors) is
 *   that call's, bit for bit -- the observed launch is the same;
 *   the FROZEN SOLVE at c starts from h_s = c, h_k = (sum_v x_v) / (|C_n| - 1) on C_n \ {s} and exactly 0.0 off C_n; every step
 *   applies the refit's update factors with the SALNMF_EPSILON clip to the members of C_n \ {s} only, h_s is never touched; the
 *   objective is the sample's KL divergence at the whole h, the stop rule the refit's.  Its error is f(c), and g(c) = f(c) - f1
 *   (one rounded subtraction).  At c = 0.0 it is bit for bit salnmf_signature_presence's null solve and g(0) its statistic.
 * salnmf_profile_likelihood evaluates g on given values: values holds n_values doubles used for every pair (values_per_pair
 * = 0) or n_samples x n_test x n_values (values_per_pair = 1), n_values in [1, 4096], every one finite and >= 0; every solve
 * starts cold, so an entry depends on its pair and its value only.  Outputs: tested  n_samples x n_test;  profile (g),
 * profile_errors (f), n_iterations, converged  n_samples x n_test x n_values;  profile_exposures  NULL, or the same x
 * n_signatures (entry s exactly c, exactly 0.0 off C_n);  exposures  n_samples x n_signatures and errors  n_samples.  Entries of
 * an untested pair: NaN in the doubles, 0 in the integers.  timings: NULL, or 3 doubles -- milliseconds by device events of the
 * observed launch and of the profile launch, and the number of device problems (a pair's values go in runs of 8).
 * Refused on the host before any launch, status 1 and salnmf_last_error: what salnmf_signature_presence refuses of these
 * arguments; n_values outside [1, 4096]; values_per_pair not 0 or 1; a value that is not finite or is negative. */
int salnmf_profile_likelihood(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                              int n_signatures, const int* test, int n_test, const uint8_t* candidates, const double* values,
                              int n_values, int values_per_pair, int min_iterations, int max_iterations, int conv_test_freq,
                              double tol, uint8_t* tested, double* profile, double* profile_errors, int* n_iterations,
                              int* converged, double* profile_exposures, double* exposures, double* errors, double* timings);

/* salnmf_exposure_intervals searches the two ends of { c : g(c) <= max_kl_increase } on the device, every trial a frozen solve
 * from a cold start and all search arithmetic in fp64; a comparison with a NaN is false.  With hh = h1[s], D = max_kl_increase,
 * J = n_bisections, E = max_expansions and g0 = statistic[n, j] = g(0):
 *   lower end: g0 <= D gives exactly 0.0 without a trial.  Otherwise lo = 0.0, hi = hh; J times m = 0.5 (lo + hi), g(m) > D ?
 *   lo = m : hi = m.  While lo is still 0.0 after them (the root lies below hh / 2^J) the halving goes on, at most E more
 *   times, and stops at the first trial with g(m) > D; lower = lo.  So lower == 0.0 with g0 > D only if none of J + E halvings
 *   of [0, hh] found a value outside.
 *   upper end: d = hh > 1.0 ? hh : 1.0, lo = hh; expansion trial e = 0, 1, .. is c = hh + d 2^e; g(c) > D ? hi = c and the
 *   expansion stops : lo = c.  After E trials without a bracket upper = +inf, bracketed = 0, no bisection.  Otherwise J times
 *   m = 0.5 (lo + hi), g(m) > D ? hi = m : lo = m; upper = hi.
 * Both ends are the outer ends of their last bracket: the interval returned contains the exact one.  lower == 0.0, that is g0 <= D,
 * is the criterion on which salnmf_assign_signatures removes a signature at max_kl_increase = D.
 * Outputs, n_samples x n_test: tested, lower, upper, estimate (hh), bracketed (1 / 0), statistic (g0), null_errors (f(0));
 * n_trials  the same x 2 (lower, upper);  exposures, errors as above;  trace_values, trace_profile  both NULL, or n_samples x
 * n_test x 2 x (E + J): the trial values and their g in trial order, NaN past n_trials.  Entries of an untested pair: NaN in the
 * doubles, 0 elsewhere.  timings as above (a problem is one end of one pair).
 * Refused on the host before any launch: what salnmf_profile_likelihood refuses of the shared arguments; max_kl_increase not
 * finite or negative; n_bisections outside [0, 64]; max_expansions outside [1, 1000]; one trace output without the other. */
int salnmf_exposure_intervals(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                              int n_signatures, const int* test, int n_test, const uint8_t* candidates, double max_kl_increase,
                              int n_bisections, int max_expansions, int min_iterations, int max_iterations, int conv_test_freq,
                              double tol, uint8_t* tested, double* lower, double* upper, double* estimate, uint8_t* bracketed,
                              int* n_trials, double* statistic, double* null_errors, double* exposures, double* errors,
                              double* trace_values, double* trace_profile, double* timings);

/* ---- Which exposures trade against each other in a sample?  The information matrix of the sample's exposures at the fit, its
 * inverse, and what the inverse says about confounding (csrc/salnmf_information.h).  counts, signatures
 * as salnmf_refit_exposures (the counts clipped to SALNMF_EPSILON, the signature rows used as given); exposures  n_samples x
 * n_signatures, finite and >= 0;  active  n_samples x n_signatures bytes, anything but 0 is "active".  Per sample:
 *   p_v = max(sum_k W[k, v] h_k, SALNMF_EPSILON) over ALL k;  d_v = x_v / p_v^2 (information = 0, observed: the Hessian of the
 *   sample's KL divergence) or 1 / p_v (information = 1, expected);  J[k, l] = sum_v W[k, v] W[l, v] d_v on the active k, l;
 *   C = D^-1/2 J D^-1/2 with D = diag(J);  C = L L^T in the natural order of k without pivoting;  min_pivot_value is the
 *   smallest L[k, k]^2, and the sample is SINGULAR at the first squared pivot <= min_pivot (min_pivot_value is then that pivot).
 * Outputs, n_samples x n_signatures: standard_errors = sqrt((C^-1)_kk / J_kk);  inflation = (C^-1)_kk;  information_diag = J_kk;
 * max_abs_correlation and most_confounded: the largest |corr_kl| over the active l != k and its index, the smallest on a tie,
 * corr_kl = (C^-1)_kl / sqrt((C^-1)_kk (C^-1)_ll) -- NaN and -1 where k is inactive, the sample is singular, or k is the only
 * active signature.  The three others are NaN where k is inactive or the sample is singular.  n_samples: min_pivot_value (NaN
 * without an active signature), singular (1 / 0), n_active.  correlation  NULL, or n_samples x n_signatures x n_signatures:
 * corr with a unit diagonal on the active set, NaN elsewhere, symmetric bit for bit; it is produced in chunks of samples whose
 * device buffer stays within chunk_bytes (0 or less: 256 MiB).  A sample's results depend on that sample alone.  timings: NULL,
 * or 2 doubles -- milliseconds by device events of the kernel launches, and the number of launches.
 * Refused on the host before any launch, status 1 and salnmf_last_error: a null argument other than correlation and timings;
 * n_samples outside [1, 2^31), n_features or n_signatures outside [1, 96]; counts, signatures or exposures that are not finite or
 * are negative, a signature without a positive sum; information not 0 or 1; min_pivot not finite or outside (0, 1). */
int salnmf_exposure_covariance(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                               int n_signatures, const double* exposures, const unsigned char* active, int information,
                               double min_pivot, int64_t chunk_bytes, double* standard_errors, double* inflation,
                               double* information_diag, double* max_abs_correlation, int* most_confounded,
                               double* min_pivot_value, int* singular, int* n_active, double* correlation, double* timings);

/* ---- Have the exposure SHARES changed between two samples of one patient?  A likelihood-ratio test of "same shares, free
 * totals" against "own exposures" per pair of rows, with a parametric-bootstrap null (csrc/salnmf_change.h, DESIGN.md section
 * 21).  Row n of counts_a and row n of counts_b form pair n: both n_samples x n_features (the second shape is passed and must
 * agree).  signatures, candidates, the iteration arguments, max_iterations % conv_test_freq == 0, n_draws, seed and chunk_bytes as
 * salnmf_signature_presence; candidates holds one set C_n per pair, for both samples and for the pooled fit.  Contract, for pair n
 * with clipped rows x_a, x_b (each max(row, SALNMF_EPSILON)):
 *   solve a, solve b and the pooled solve are salnmf_signature_presence's SOLVE ON A SET C_n of x_a, of x_b and of the row
 *   x_p[v] = x_a[v] + x_b[v], each from a cold start -- bit for bit the exposures, error, iteration count and convergence flag
 *   of salnmf_assign_signatures_ex with candidates = required = C_n on that row: (h_a, f_a), (h_b, f_b), (h_0, f_p);
 *   with t the rows' sums, c_a = t_a / (t_a + t_b), c_b = t_b / (t_a + t_b) and P_0 = h_0 W as the pooled solve holds it at its
 *   stopping test: g_a = KL(x_a || c_a P_0), g_b = KL(x_b || c_b P_0), the refit's objective term by term;
 *   statistic[n] = (g_a - f_a) + (g_b - f_b), half the likelihood-ratio statistic;
 *   the pair is UNTESTED if C_n has fewer than two members or either row's integer total is 0: tested[n] = 0, it draws nothing
 *   and costs no solve;
 *   null draw b of the pair is two model draws (salnmf_draw_model_counts' steps) from the exposures h_0, one of sum_v counts_a[n, v]
 *   trials and one of sum_v counts_b[n, v], with the Philox counter (q, 0x43480000 + side, n, b), side 0 for a and 1 for b: a
 *   stream family of its own ("CH" in the upper half of the second word), so the draws of a pair depend on (seed, n, side, b) and
 *   on h_0 only;
 *   every draw pair goes through the same three solves and the same two divergences: null_statistics[b, n];
 *   reduction as salnmf_signature_presence: n_exceed[n] counts null_statistics[b, n] >= statistic[n] (false for a NaN on either
 *   side), null_mean[n] is their sum from 0.0 in ascending b, divided by n_draws.  The p-value is (1 + n_exceed) / (n_draws + 1).
 * Outputs: tested (1 / 0), statistic, n_exceed, null_mean  n_samples;  exposures_a (h_a), exposures_b (h_b), pooled_exposures (h_0)
 * n_samples x n_signatures;  errors  n_samples x 3 (f_a, f_b, f_p);  null_errors  n_samples x 2 (g_a, g_b);  n_iterations, converged
 * n_samples x 3 (a, b, pooled);  null_statistics  n_draws x n_samples;  null_n_iterations  n_draws x n_samples x 3;  draws  NULL, or
 * n_draws x n_samples x 2 x n_features, plain counts.  Entries of an untested pair: NaN in the doubles (0 in draws), 0 in the
 * integers.  timings: NULL, or 4 doubles -- milliseconds by device events of the draw launches, the solve launches and the
 * reduction, and the number of chunks.
 * Refused on the host before any launch, status 1 and salnmf_last_error: a null argument other than candidates, draws and
 * timings; shapes that differ; what salnmf_signature_presence refuses of these arguments, for either count matrix. */
int salnmf_exposure_change(int device, const double* counts_a, int64_t n_samples, int n_features, const double* counts_b,
                           int64_t n_samples_b, int n_features_b, const double* signatures, int n_signatures,
                           const uint8_t* candidates, int n_draws, uint64_t seed, int min_iterations, int max_iterations,
                           int conv_test_freq, double tol, int64_t chunk_bytes, uint8_t* tested, double* statistic, int* n_exceed,
                           double* null_mean, double* exposures_a, double* exposures_b, double* pooled_exposures, double* errors,
                           double* null_errors, int* n_iterations, int* converged, double* null_statistics,
                           int* null_n_iterations, double* draws, double* timings);

/* ---- WHICH signature's share has changed between the two samples of a pair?  A likelihood-ratio test of "signature s has the
 * same share in both samples, everything else free" against "own exposures", per (pair, tested signature), with a
 * parametric-bootstrap null (csrc/salnmf_sigchange.h).  counts_a, counts_b, signatures, candidates, the
 * iteration arguments, n_draws, seed and chunk_bytes as salnmf_exposure_change; test as salnmf_signature_presence (n_test distinct
 * indices).  Contract, for pair n with clipped rows x_a, x_b, candidate set C_n and s = test[j]:
 *   t_a, t_b are the clipped rows' sums, c_a = t_a / (t_a + t_b), c_b = t_b / (t_a + t_b); the share of s in a sample is h_s / t;
 *   solves a and b are salnmf_exposure_change's: (h_a, f_a), (h_b, f_b);
 *   the TIED solve runs both samples side by side from the cold start h_k = t_side / |C_n|: every entry but s takes its own
 *   sample's update factor, entry s takes F = c_a u_as + c_b u_bs, evaluated as (u_as + u_bs) / 2 + ((c_a - c_b) / 2) (u_as - u_bs) with every operation
 *   rounded on its own (so that equal factors give that factor, and the two samples can be exchanged), in both samples; the
 *   EPSILON clip is per sample; the objective f_a0 + f_b0 (one rounded sum) is tested at iteration 0 and at every multiple of
 *   conv_test_freq by the family's stop rule, and both samples stop together: (h_a0, f_a0), (h_b0, f_b0);
 *   statistic[n, j] = (f_a0 - f_a) + (f_b0 - f_b), half the likelihood-ratio statistic with one constrained parameter; exchanging
 *   counts_a and counts_b exchanges the sides' results and leaves its bits;
 *   the problem is UNTESTED if s is not in C_n, C_n has fewer than two members or either row's integer total is 0: tested[n, j] = 0,
 *   it draws nothing and costs no solve;
 *   null draw b of the problem is two model draws (salnmf_draw_model_counts' steps), side a from the exposures h_a0 with
 *   sum_v counts_a[n, v] trials and side b from h_b0 with sum_v counts_b[n, v], under the Philox counter
 *   (q, 0x53430000 + 2 s + side, n, b): a stream family of its own ("SC" in the upper half of the second word);
 *   every draw pair goes through the same three solves: null_statistics[b, n, j]; reduction as salnmf_signature_presence.
 * Outputs: tested (1 / 0), statistic, n_exceed, null_mean  n_samples x n_test;  exposures_a (h_a), exposures_b (h_b)  n_samples x
 * n_signatures (NaN rows where no problem of the pair is tested);  tied_exposures_a (h_a0), tied_exposures_b (h_b0)  n_samples x n_test
 * x n_signatures;  errors  n_samples x n_test x 4 (f_a, f_b, f_a0, f_b0);  n_iterations, converged  n_samples x n_test x 3 (a, b,
 * tied);  null_statistics  n_draws x n_samples x n_test;  null_n_iterations  n_draws x n_samples x n_test x 3;  draws  NULL, or n_draws
 * x n_samples x n_test x 2 x n_features, plain counts.  Entries of an untested problem: NaN in the doubles (0 in draws), 0 in the
 * integers.  timings: NULL, or 4 doubles -- milliseconds by device events of the draw launches, the solve launches and the
 * reduction, and the number of chunks.
 * Refused on the host before any launch, status 1 and salnmf_last_error: a null argument other than candidates, draws and
 * timings; shapes that differ; what salnmf_exposure_change and salnmf_signature_presence refuse of these arguments. */
int salnmf_signature_change(int device, const double* counts_a, int64_t n_samples, int n_features, const double* counts_b,
                            int64_t n_samples_b, int n_features_b, const double* signatures, int n_signatures, const int* test,
                            int n_test, const uint8_t* candidates, int n_draws, uint64_t seed, int min_iterations,
                            int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes, uint8_t* tested,
                            double* statistic, int* n_exceed, double* null_mean, double* exposures_a, double* exposures_b,
                            double* tied_exposures_a, double* tied_exposures_b, double* errors, int* n_iterations, int* converged,
                            double* null_statistics, int* null_n_iterations, double* draws, double* timings);

/* ---- Refit of exposures to FIXED signatures under a NEGATIVE-BINOMIAL likelihood: counts overdispersed around h W with variance
 * p + p^2 / alpha (csrc/salnmf_nb.h).  counts, signatures, the problems (dataset -1 the counts, dataset r
 * resample r of salnmf_resample_counts(counts, n_resamples, seed)), the iteration arguments, the quantiles, chunk_bytes, every
 * output and timings as salnmf_refit_exposures.  dispersion  n_samples: sample n's alpha, which its resamples carry too.
 *   x = max(row, SALNMF_EPSILON);  h_k = (sum_v x_v) / n_signatures;
 *   step (update_H, _utils_klnmf.py:258-264, with the negative binomial's second product): p = h W, a_v = x_v / p_v,
 *   b_v = (x_v + alpha) / (p_v + alpha), h_k <- max((h_k sum_v W[k, v] a_v) / (sum_v W[k, v] b_v), SALNMF_EPSILON);
 *   objective: sum_v [ x_v log(x_v / p_v) - (x_v + alpha) log((x_v + alpha) / (p_v + alpha)) ] -- not negative, 0 at p = x, the KL
 *   divergence as alpha -> infinity -- at iteration 0 and every multiple of conv_test_freq; stop rule, latching, converged and
 *   n_iterations as salnmf_refit_exposures.  errors and errors_resampled hold this divergence.
 * Refused on the host before any launch, status 1 and salnmf_last_error: what salnmf_refit_exposures refuses, a null dispersion,
 * and a dispersion that is not finite or lies outside (0, 1e6] (towards infinity the second logarithm's argument is 1 to
 * rounding; salnmf_refit_exposures is the limit). */
int salnmf_nb_refit_exposures(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                              int n_signatures, const double* dispersion, int n_resamples, uint64_t seed, int n_quantiles,
                              const double* quantiles, int min_iterations, int max_iterations, int conv_test_freq, double tol,
                              int64_t chunk_bytes, double* exposures, double* errors, int* n_iterations, int* converged,
                              double* exposures_quantiles, double* exposures_mean, int* n_iterations_resampled,
                              double* errors_resampled, double* exposures_resampled, double* timings);

/* ---- Draws from a FITTED negative-binomial model and the goodness-of-fit test they calibrate (csrc/salnmf_nbdraw.h, DESIGN.md
 * section 24).  out  n_draws x n_samples x n_features: row n of draw b is one gamma-Poisson draw around exposures[n, :] @ signatures
 * with dispersion[n] -- unconditional, the row total varies -- bit for bit by the contract of section 24:
 *   P_v = sum_k h_k W[k, v] (ascending k, product then sum, no fused multiply-add);  lambda_v = g_v (P_v / alpha), g_v ~ Gamma(alpha, 1)
 *   by Marsaglia-Tsang with a polar normal;  Lambda = sum_v lambda_v (ascending v);  T ~ Poisson(Lambda) by counted exponentials
 *   below 10 and Hoermann's PTRS from 10 on;  T trials over the 40-bit table of lambda_v / Lambda as salnmf_draw_model_counts places
 *   them.  Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter (q, 0x4E420000 + stream, n, b).  Draw b does not depend on
 *   n_draws.  signatures as given (rows of sum one expected, not normalised here).
 * n_failed  one int: rows written as zeros because 64 gamma attempts, 128 exponentials or 64 PTRS attempts were all rejected (each
 *   below 2^-100) or because Lambda reached 2^31; the status is 0 all the same, and a caller treats n_failed != 0 as an error.
 * Refused on the host before any launch, status 1 and salnmf_last_error: a null argument; n_samples outside [1, 2^31); n_features
 * or n_signatures outside [1, 96]; n_draws outside [1, 65536]; exposures or signature entries that are not finite or are negative;
 * a row with sum_v P_v above 2^24; a dispersion that is not finite or lies outside (0, 1e6]. */
int salnmf_draw_nb_counts(int device, const double* exposures, int64_t n_samples, int n_signatures, const double* signatures,
                          int n_features, const double* dispersion, int n_draws, uint64_t seed, double* out, int* n_failed);

/* The parametric-bootstrap test of section 16 under the negative-binomial model.  The observed fit is salnmf_nb_refit_exposures
 * (n_resamples = 0) bit for bit; draw b is salnmf_draw_nb_counts of those exposures, read where the refit left them on the device,
 * with the samples' own dispersions, written as max(count, SALNMF_EPSILON); its refit is salnmf_nb_refit_exposures of the draw with
 * the same dispersions and iteration arguments; n_exceed[n] counts null_errors[b, n] >= errors[n] (false for a NaN) and null_mean[n]
 * is their sum in ascending b over n_draws.  null_errors, null_n_iterations  n_draws x n_samples.  draws  n_draws x n_samples x
 * n_features or null.  timings  4 doubles or null: device-event ms of the draw launches, the refit launches and the reduction, and
 * the chunk count.  n_failed as above.  Refused: what salnmf_nb_refit_exposures refuses, n_draws outside [1, 65536], counts that are
 * not integers, and a row total above 2^24. */
int salnmf_nb_goodness_of_fit(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                              int n_signatures, const double* dispersion, int n_draws, uint64_t seed, int min_iterations,
                              int max_iterations, int conv_test_freq, double tol, int64_t chunk_bytes, double* exposures,
                              double* errors, int* n_iterations, int* converged, int* n_exceed, double* null_mean,
                              double* null_errors, int* null_n_iterations, double* draws, double* timings, int* n_failed);

/* ---- sparse assignment under the negative-binomial likelihood.
 *
 * salnmf_assign_signatures_ex with the step and the divergence of salnmf_nb_refit_exposures: every argument and output means what
 * it means there, `dispersion` holds one alpha per sample (a resample of sample n carries sample n's), errors / kl_increase /
 * kl_decrease are negative-binomial divergences and their differences -- log-likelihood differences of one sample at one alpha,
 * so max_kl_increase keeps its meaning.  Contract, for problem p (sample n or a resample of it), C_n the candidates (all K if
 * null), R_n the required subset (none if null):
 *   x = max(row, SALNMF_EPSILON);  h0 = (sum_v x_v) / |C_n|;  h = h0 on C_n and exactly 0.0 elsewhere;
 *   a SOLVE iterates the entries that are not 0.0:  p = h W, a_v = x_v / p_v, b_v = (x_v + alpha) / (p_v + alpha),
 *     un_k = sum_v W_kv a_v, ud_k = sum_v W_kv b_v, h_k <- max((h_k un_k) / ud_k, SALNMF_EPSILON); tested on the negative-binomial
 *     divergence at iteration 0 and every multiple of conv_test_freq counted from the solve's start; the stop rule of section 14;
 *   phase 0 solves on C_n (dense_*: with no sets, salnmf_nb_refit_exposures bit for bit); backward rounds as section 14 with the
 *     protected set starting as R_n; with readd the re-addition pass of section 14.1, its selection factor u_k = un_k / ud_k at the
 *     accepted h (one division; not the step's quantity), largest first, lowest index on equal values, tried only if u_k > 1.
 * candidates = required = A is the solve on the active set A: no trial, exposures = dense_exposures.
 * Refused (status 1, before any launch, nothing written): what salnmf_assign_signatures_ex refuses, a null dispersion, and a
 * dispersion that is not finite or lies outside (0, 1e6]. */
int salnmf_nb_assign_signatures(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                                int n_signatures, const double* dispersion, int n_resamples, uint64_t seed, int n_quantiles,
                                const double* quantiles, int min_iterations, int max_iterations, int conv_test_freq, double tol,
                                double max_kl_increase, int64_t chunk_bytes, const uint8_t* candidates, const uint8_t* required, int readd,
                                double* exposures, int* active, double* errors, int* removal_round, double* kl_increase, int* n_trials,
                                int64_t* n_iterations, int* converged, double* dense_exposures, double* dense_errors,
                                int* dense_n_iterations, int* dense_converged, double* selection_frequency, double* exposures_quantiles,
                                double* exposures_mean, double* exposures_resampled, int* readd_round, double* kl_decrease,
                                double* timings);

/* ---- Is signature s present in this sample, under the negative-binomial model?  (csrc/salnmf_nb_presence.h)
 * salnmf_signature_presence with the step and the divergence of salnmf_nb_refit_exposures and the draw of salnmf_draw_nb_counts:
 * every argument and output means what it means there, `dispersion` holds one alpha per sample.  Contract, for sample n with
 * alpha_n, candidate set C_n and s = test[j]:
 *   a SOLVE ON A SET A is salnmf_nb_assign_signatures with candidates = required = A, bit for bit: exposures, error, iteration
 *   count and convergence flag;
 *   the alternative is the solve on C_n (h1, f1), the null the solve on C_n \ {s} (h0, f0); statistic[n, j] = f0 - f1, one rounded
 *   subtraction of two negative-binomial divergences at alpha_n: a log-likelihood difference, half the likelihood-ratio statistic;
 *   UNTESTED pairs as salnmf_signature_presence;
 *   null draw b of the pair is one draw of salnmf_draw_nb_counts' contract from the exposures h0 and alpha_n, with the Philox
 *   counter (q, 0x4E420000 + stream, n, ((s + 1) << 16) | b): b < 65536 fills the low half of the draw word and s + 1 the bits
 *   above, so no pair's draws coincide with another's or with salnmf_draw_nb_counts' / salnmf_nb_goodness_of_fit's (upper half 0);
 *   they depend on (seed, n, s, b), h0 and alpha_n only.  The draw is UNCONDITIONAL: null totals vary, as in
 *   salnmf_nb_goodness_of_fit, written as max(count, SALNMF_EPSILON);
 *   every draw goes through the same two solves from cold starts with alpha_n; the reduction is salnmf_signature_presence's.
 * n_failed as salnmf_draw_nb_counts'.  timings as salnmf_signature_presence's.
 * Refused, status 1 and salnmf_last_error: what salnmf_signature_presence refuses; a null dispersion or n_failed; a dispersion
 * that is not finite or lies outside (0, 1e6] (all of these before any launch); and, after the observed launch and before any draw,
 * a null fit h0 with sum_v (h0 W)_v above 2^24. */
int salnmf_nb_signature_presence(int device, const double* counts, int64_t n_samples, int n_features, const double* signatures,
                                 int n_signatures, const double* dispersion, const int* test, int n_test, const uint8_t* candidates,
                                 int n_draws, uint64_t seed, int min_iterations, int max_iterations, int conv_test_freq, double tol,
                                 int64_t chunk_bytes, uint8_t* tested, double* statistic, int* n_exceed, double* null_mean,
                                 double* exposures, double* errors, double* null_exposures, double* null_errors, int* n_iterations,
                                 int* converged, double* null_statistics, int* null_n_iterations, double* draws, double* timings,
                                 int* n_failed);

#ifdef __cplusplus
}
#endif
#endif /* SALNMF_H */
