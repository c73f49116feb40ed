"""Every instantiation and every shape edge of the refit family (DESIGN.md sections 13-20) against its reference.

The kernels of ``csrc/salnmf_refit.h`` are templates over KT = ceil(K / 16) = 1..6 and mask their pads with ``k < K`` and
``16 vt + 4 r + q < V``.  One list of (K, V) puts every KT at its lower edge, at its upper edge and once inside, and every edge
of the feature axis at least twice; N = 40 problems throughout (two full tiles and one of 8).

    K   V   KT   K edge               V edge                         | (K, V) KT  candidate-word edge
    15   1   1   upper - 1            a single feature               | 31 96  2   m = 31
    16  16   1   upper                exactly one tile               | 32 96  2   m = 32: ~0u
    32  15   2   upper, word 0 full   one short of a tile            | 63 96  4   m = 31 in word 1
    33  17   3   lower, bit 0 word 1  one past a tile                | 64 96  4   m = 32 in word 1: ~0u
    40  96   3   interior             no pad
    47  96   3   upper - 1            no pad
    48  83   3   upper                a cut inside tile 5
    49  16   4   lower                exactly one tile
    64  95   4   upper, word 1 full   one short of the last tile
    65  95   5   lower, bit 0 word 2  one short of the last tile
    70  96   5   interior             no pad
    80  33   5   upper                one past two tiles
    81  96   6   lower                no pad
    95  83   6   upper - 1            a cut inside tile 5

What is compared, kernel by kernel, at KT = 1..6 and V in {1, 15/16/17, 33, 83, 95, 96}:

    refit_kernel               exposures, objective, n_iterations at T = 200 against the longdouble replica: every shape; two
                               convergence cases at KT = 3 and 5
    assign_kernel<KT, false>   decisions and values against the replica of section 14: every shape but (15, 1); at (15, 1)
                               phase 0 alone, against the longdouble refit replica
    assign_kernel<KT, true>    the same with candidate sets and the re-addition pass: every shape but (15, 1), and the four
                               candidate-word edges; at (15, 1) phase 0 alone, against the refit on the sub-catalogue
    presence_kernel            observed statistic, both errors, both exposures at 20-step solves against the replica; the
                               draws, bit for bit: every shape and the four candidate-word edges
    power (presence_kernel)    n_detected against the presence test's rule on the kept draws, bit for bit: the same
    profile_kernel             the frozen solves against the replica: the same
    change_kernel              the replica comparisons of tests/test_gpu_change.py -- the null divergences against longdouble,
                               the draws bit for bit, the null statistics on the kept draws -- with its checks of the three
                               fits and of the reduction: the same
    sigchange_kernel           the replica comparisons of tests/test_gpu_sigchange.py -- the tied solve at 40 steps against
                               longdouble, the draws bit for bit, the null statistics on the kept draws -- with its checks of
                               the free fits and of the reduction: the same
    information_kernel         exposure_covariance against the long-double contract: every shape
    independence               a row subset against the full call, bit for bit: one shape per KT, refit, assign and presence
    pads                       inputs cut out of wider arrays whose other columns hold NaN: (33, 17) and (80, 33)

(15, 1) has no elimination to compare: with one feature every signature is the vector [1.0] and every exposure of a sample is
the same number in every replica, so every arg-min is a K-way tie and no decision is isolated.  What does not depend on the
ties, phase 0, is compared there.

No bound is chosen here.  Each is a recorded yardstick of the project times its margin of 16 -- ``test_gpu_refit.H_SPREAD`` and
``G_RAW``, ``_assign_masks_ref.H_SPREAD`` / ``F_SPREAD``, ``_change_ref.G_SPREAD``, ``_sigchange_ref.H_SPREAD`` / ``F_SPREAD`` --
or, for the covariance, the deviation of the float64 replicas from the long-double reference measured on the case's own inputs
(``COV_MEASURED``).  tests/test_family_edges_host.py measures all of them on the CPU on these very inputs and fails when a case
exceeds its record, or is vacuous.  Where a case's own float64 spread exceeds the recorded constant, ``F_SPREAD_OF``,
``CHANGE_G_SPREAD_OF`` and ``SIGCHANGE_SPREAD_OF`` hold the case's measured value for the host test; the device stays held to
16 x the recorded constant, the smaller of the two.
"""

import functools

import numpy as np
import pytest

import _assign_masks_ref as mref
import _assign_ref as aref
import _cov_ref as cov_ref
import _power_ref as power_ref
import _presence_ref as presence_ref
import _profile_ref as profile_ref
import _refit_ref as ref
import salamander_amd as sal
import test_gpu_assign as tga
import test_gpu_assign_masks as tgm
import test_gpu_change as tgch
import test_gpu_covariance as tgc
import test_gpu_profile as tgprof
import test_gpu_refit as tgr
import test_gpu_sigchange as tgsc

pytestmark = pytest.mark.gpu

EPS = ref.EPSILON
N = 40
SHAPES = [(15, 1), (16, 16), (32, 15), (33, 17), (40, 96), (47, 96), (48, 83), (49, 16), (64, 95), (65, 95), (70, 96), (80, 33), (81, 96), (95, 83)]
WORD_EDGES = [(31, 96), (32, 96), (63, 96), (64, 96)]  # (1u << m) - 1u gives way to ~0u at m = 32: for the kernels that pass a candidate set
ASSIGN_SHAPES = SHAPES[1:]
ONE_PER_KT = [(16, 16), (32, 15), (48, 83), (49, 16), (65, 95), (95, 83)]
PAD_SHAPES = [(33, 17), (80, 33)]
# (N, K) of test_gpu_refit.test_convergence_of_every_problem at KT = 3 and 5.  The deviation of the float64 replicas' relative
# change from the longdouble one's, whose record is test_gpu_refit.G_RAW = 2.0e-7, is 1.4e-7 to 5.1e-7 over K = 33..48 and
# 65..80 at N = 32 and exceeds the record at most of them (a finding noted next to G_RAW too); these two hold it with the most
# room, measured 1.44e-7 and 1.76e-7 over every eligible test up to max_iterations (tests/test_family_edges_host.py)
CONVERGENCE = [(32, 35), (32, 80)]
THR = tga.THR
FIXED = mref.FIXED  # the assignment's solves: 20 steps each
STEPS = tgprof.STEPS  # the pair kernels' solves against a replica: 20 steps each
FIT = dict(min_iterations=20, max_iterations=60, conv_test_freq=10, tol=1e-5)  # the convergence rule: problems of a tile stop at different tests
CONVERGING = tgm.CONVERGING
B, A, SHARES, ALPHA = 3, 2, (0.0, 0.25), 0.5
SEED = 12345678901234567
# (K, V, kind) -> the case's own float64 spread of f about the longdouble replica where it exceeds _assign_masks_ref.F_SPREAD = 3.5e-16
# (measured on the CPU by tests/test_family_edges_host.py, rounded up to two digits; the measured figure beside it)
F_SPREAD_OF = {
    (16, 16, "plain"): 4.2e-16,  # measured 4.10e-16
    (65, 95, "plain"): 4.1e-16,  # measured 4.01e-16
    (95, 83, "plain"): 6.8e-16,  # measured 6.78e-16
    (16, 16, "masked"): 4.2e-16,  # measured 4.10e-16
    (33, 17, "masked"): 6.8e-16,  # measured 6.72e-16
    (49, 16, "masked"): 3.8e-16,  # measured 3.79e-16
    (64, 95, "masked"): 4.8e-16,  # measured 4.74e-16
    (65, 95, "masked"): 5.2e-16,  # measured 5.14e-16
    (70, 96, "masked"): 4.6e-16,  # measured 4.59e-16
    (95, 83, "masked"): 4.4e-16,  # measured 4.32e-16
    (32, 96, "masked"): 4.7e-16,  # measured 4.61e-16
    (64, 96, "masked"): 3.7e-16,  # measured 3.68e-16
}
# (K, V) -> the case's own float64 spread of g_a, g_b where it exceeds _change_ref.G_SPREAD = 1.5e-16 (``_change_ref.g_spread``)
CHANGE_G_SPREAD_OF = {
    (32, 15): 1.6e-16,  # measured 1.53e-16
    (48, 83): 1.8e-16,  # measured 1.70e-16
    (49, 16): 1.6e-16,  # measured 1.57e-16
    (64, 95): 3.3e-16,  # measured 3.25e-16
    (65, 95): 2.1e-16,  # measured 2.00e-16
    (95, 83): 1.9e-16,  # measured 1.87e-16
    (31, 96): 2.1e-16,  # measured 2.07e-16
    (64, 96): 1.8e-16,  # measured 1.75e-16
}
# (K, V, "h" or "f") -> the tied solve's own float64 spread where it exceeds _sigchange_ref.H_SPREAD = 1.5e-14 or F_SPREAD = 2.1e-16
# (``_sigchange_ref.fixed_spread``)
SIGCHANGE_SPREAD_OF = {
    (47, 96, "h"): 1.7e-14,  # measured 1.65e-14
    (64, 95, "f"): 2.7e-16,  # measured 2.62e-16
    (65, 95, "f"): 2.5e-16,  # measured 2.46e-16
}
# (K, V, information) -> (relative, absolute): the four float64 replicas' largest deviation from the long-double reference on the
# case's own inputs, rounded up to two digits (tests/test_family_edges_host.py::test_covariance_records_hold measures them)
COV_MEASURED = {
    (15, 1, "observed"): (5e-16, 0),  # measured 4.97e-16, 0; singular 2
    (15, 1, "expected"): (2.7e-16, 0),  # measured 2.61e-16, 0; singular 2
    (16, 16, "observed"): (7.2e-10, 1.4e-10),  # measured 7.15e-10, 1.31e-10; singular 0
    (16, 16, "expected"): (1.7e-15, 8.5e-16),  # measured 1.62e-15, 8.42e-16; singular 0
    (32, 15, "observed"): (8.5e-15, 1.5e-15),  # measured 8.46e-15, 1.49e-15; singular 2
    (32, 15, "expected"): (4.1e-15, 7.4e-16),  # measured 4.02e-15, 7.31e-16; singular 2
    (33, 17, "observed"): (8.2e-15, 2.1e-15),  # measured 8.11e-15, 2.03e-15; singular 2
    (33, 17, "expected"): (7.3e-15, 1.6e-15),  # measured 7.26e-15, 1.55e-15; singular 2
    (40, 96, "observed"): (5.1e-15, 3.7e-15),  # measured 5.09e-15, 3.69e-15; singular 0
    (40, 96, "expected"): (1.5e-15, 4.3e-16),  # measured 1.46e-15, 4.25e-16; singular 0
    (47, 96, "observed"): (5.6e-15, 2.4e-15),  # measured 5.53e-15, 2.32e-15; singular 0
    (47, 96, "expected"): (1.6e-15, 6.3e-16),  # measured 1.57e-15, 6.29e-16; singular 0
    (48, 83, "observed"): (1.7e-14, 5.7e-15),  # measured 1.66e-14, 5.66e-15; singular 0
    (48, 83, "expected"): (1.9e-15, 5.9e-16),  # measured 1.84e-15, 5.8e-16; singular 0
    (49, 16, "observed"): (5.8e-14, 1.1e-14),  # measured 5.73e-14, 1.02e-14; singular 2
    (49, 16, "expected"): (1.3e-14, 2.6e-15),  # measured 1.23e-14, 2.54e-15; singular 2
    (64, 95, "observed"): (1.7e-15, 7.1e-16),  # measured 1.68e-15, 7.07e-16; singular 0
    (64, 95, "expected"): (2e-15, 7.5e-16),  # measured 1.94e-15, 7.46e-16; singular 0
    (65, 95, "observed"): (2.2e-15, 7.8e-16),  # measured 2.17e-15, 7.79e-16; singular 0
    (65, 95, "expected"): (2e-15, 7.7e-16),  # measured 1.92e-15, 7.65e-16; singular 0
    (70, 96, "observed"): (2.1e-15, 6.9e-16),  # measured 2.03e-15, 6.83e-16; singular 0
    (70, 96, "expected"): (1.8e-15, 6.5e-16),  # measured 1.71e-15, 6.5e-16; singular 0
    (80, 33, "observed"): (9.8e-15, 1.9e-15),  # measured 9.79e-15, 1.82e-15; singular 2
    (80, 33, "expected"): (1.6e-14, 2.3e-15),  # measured 1.59e-14, 2.26e-15; singular 2
    (81, 96, "observed"): (2.1e-15, 7.2e-16),  # measured 2.07e-15, 7.11e-16; singular 0
    (81, 96, "expected"): (1.8e-15, 6.2e-16),  # measured 1.73e-15, 6.11e-16; singular 0
    (95, 83, "observed"): (1.2e-14, 8.4e-16),  # measured 1.13e-14, 8.36e-16; singular 2
    (95, 83, "expected"): (8.8e-15, 7.5e-16),  # measured 8.78e-15, 7.43e-16; singular 2
}


# ---- inputs

def refit_case(K, V):
    return tgr.catalogue(N, K, V, seed=K + V)


def plain_case(K, V):
    """(P, K, V, seed) of ``test_gpu_assign.replicas``."""
    return N, K, V, 0


def masked_case(K, V):
    """A case of ``_assign_masks_ref``: per-sample random sets that all hold signature K - 1 and signature 32 floor((K - 1) / 32),
    the re-addition pass on."""
    return N, K, V, 0, "edge", True, THR


@functools.lru_cache(maxsize=None)
def pair_case(K, V):
    """(counts, signatures, test, candidates) as ``test_gpu_presence.case`` builds them -- row totals 0, 1, 2, 257 and 100 000, a
    last signature with zeros (row 3 is drawn from it), rows 5..8 without test[0], row 9 with test[1] alone, row 10 with neither
    -- for any V (the last signature keeps at least one feature) and with the candidate-word edge: the tested signatures are 0
    and K - 1, and every set but those of rows 5..10 holds K - 1 and 32 floor((K - 1) / 32).  Never modified."""
    rng = np.random.default_rng(1000 * K + V)
    X, W = ref.poisson_catalogue(N, K, V=V, seed=70 + K, zero_heavy=3)
    W[K - 1, rng.permutation(V)[: min(max(2, V // 3), V - 1)]] = 0.0
    W = ref.normalize(W)
    X[0] = 0.0
    for row, total in ((1, 1), (2, 2), (3, 257), (4, 100000)):
        X[row] = rng.multinomial(total, W[K - 1] if row == 3 else np.full(V, 1.0 / V))
    test = [0, K - 1]
    C = rng.random((N, K)) < 0.8
    C[:, [0, 1, K - 1, 32 * ((K - 1) // 32)]] = True
    C[:5] = True
    C[5:9, 0] = False
    C[9] = False
    C[9, K - 1] = True
    C[10] = False
    C[10, 1] = True
    for a in (X, W, C):
        a.setflags(write=False)
    return X, W, test, C


def grid_of(K):
    return tgprof.grid_of(K)


@functools.lru_cache(maxsize=None)
def pair_replica(K, V):
    """The float64 replica of the pair kernels' fixed solves on ``pair_case``: the alternative fit, and the frozen solves at the
    grid's four values, of which the first is 0 -- the null fit of the presence test."""
    X, W, test, C = pair_case(K, V)
    return profile_ref.profile(X, W, test, grid_of(K), candidates=C, **STEPS)


@functools.lru_cache(maxsize=None)
def cov_case(K, V):
    """(X, W, H, active) as ``_cov_ref.gpu_case`` builds them, with an active set of at most min(V, 5) signatures per sample
    where K > V (samples 0 and 1 keep all K there: rank deficient, singular)."""
    X, W, H = cov_ref.poisson_case(N, K, V, 0, mutations=(200, 20000) if K < 64 else (2e5, 2e6))
    if K <= V:
        H[5:7] = cov_ref.restrict_support(H[5:7], max(1, K // 2), 0)
        H[7] = 0.0
        return X, W, H, cov_ref.default_active(H)
    return X, W, H, cov_ref.subset_mask(N, K, min(V, 5), 0, full=(0, 1))


@functools.lru_cache(maxsize=None)
def cov_reference(K, V, information):
    """The long-double contract on ``cov_case``; `singular` must not hinge on rounding: the smallest pivot is >= 1e-6 or exactly 0."""
    r = cov_ref.reference(*cov_case(K, V), information)
    piv = np.asarray(r.min_pivot_value, dtype=np.float64)[r.n_active > 0]
    assert ((piv >= 1e-6) | (piv == 0.0)).all(), piv.min()
    assert np.array_equal(r.singular[r.n_active > 0], piv == 0.0)
    return r


def subset_rows(n):
    """Rows that move problems into other lane columns and tiles."""
    return np.random.default_rng(n).permutation(N)[:n]


# ---- 1. refit

@pytest.mark.parametrize("K,V", SHAPES)
def test_refit_fixed_steps_entry_by_entry(K, V):
    tgr.test_fixed_steps_entry_by_entry(N, K, V)


@pytest.mark.parametrize("P,K", CONVERGENCE)
def test_refit_convergence_of_every_problem(P, K):
    tgr.test_convergence_of_every_problem(P, K)


# ---- 2. assign

@pytest.mark.parametrize("K,V", ASSIGN_SHAPES)
def test_assign_decisions_and_values(K, V):
    """``test_gpu_assign.test_decisions_and_values_against_the_replica`` at the shape, every decision isolated on the CPU, with the
    value bounds of ``_assign_masks_ref``."""
    X, W, runs = tga.replicas(*plain_case(K, V))
    a, _, ld = runs
    ok, margin = aref.isolation(runs, THR)
    assert ok.all(), np.flatnonzero(~ok)
    scale, h_spread, f_spread = tga.host_spread(X, W, runs)
    got = sal.assign_signatures(X, W, THR, **FIXED)
    for name in ("active", "removal_round", "n_trials", "n_iterations"):
        assert np.array_equal(getattr(got, name), getattr(a, name)), name
    assert np.array_equal(got.n_iterations, 20 * (got.n_trials.astype(np.int64) + 1))
    assert np.array_equal(got.converged[got.n_trials == 0], got.dense_converged[got.n_trials == 0])
    assert np.array_equal(got.exposures == 0.0, ~got.active) and np.array_equal(np.isnan(got.kl_increase), np.isnan(a.kl_increase))
    dH, dF = tga.deviations(got, ld, scale)
    print(f"assign K={K} V={V}: trials {got.n_trials.min()}..{got.n_trials.max()}, threshold margin {margin:.3g}, host spread H {h_spread:.3g} "
          f"f {f_spread:.3g}, device H {dH:.3g} f {dF:.3g}, of the bounds {dH / (16 * mref.H_SPREAD):.3g} {dF / (16 * mref.F_SPREAD):.3g}")
    assert dH <= 16 * mref.H_SPREAD
    assert dF <= 16 * mref.F_SPREAD


@pytest.mark.parametrize("K,V", ASSIGN_SHAPES + WORD_EDGES)
def test_assign_with_sets_decisions_and_values(K, V):
    """``test_gpu_assign_masks.test_decisions_and_values_against_the_replica`` at the shape."""
    case = masked_case(K, V)
    X, W, kw, runs, (ok, margin, umargin) = mref.case_replicas(*case)
    a, _, ld = runs
    assert ok.sum() >= 0.9 * ok.size
    rows = np.flatnonzero(ok)
    scale, h_spread, f_spread = mref.host_spread(X, W, runs, rows)
    got = sal.assign_signatures(X, W, **kw, **FIXED)
    C = kw["candidates"]
    assert np.array_equal(got.candidates, C) and C[:, K - 1].all() and C[:, 32 * ((K - 1) // 32)].all()
    for name in ("active", "removal_round", "n_trials", "n_iterations", "readd_round"):
        assert np.array_equal(getattr(got, name)[rows], getattr(a, name)[rows]), name
    assert np.array_equal(got.n_iterations, 20 * (got.n_trials.astype(np.int64) + 1))
    agree = ok & (runs[0].converged == runs[1].converged) & (runs[0].converged == runs[2].converged)
    assert agree.sum() >= 0.9 * agree.size and np.array_equal(got.converged[agree], a.converged[agree])
    assert np.array_equal(np.isnan(got.kl_decrease[rows]), np.isnan(a.kl_decrease[rows]))
    assert np.array_equal(np.isnan(got.kl_increase[rows]), np.isnan(a.kl_increase[rows]))
    # off the candidate set: exactly 0.0, inactive, never tried
    assert (got.exposures[~C] == 0.0).all() and not got.active[~C].any() and (got.dense_exposures[~C] == 0.0).all()
    assert np.isnan(got.kl_increase[~C]).all() and (got.removal_round[~C] == -1).all() and np.array_equal(got.exposures == 0.0, ~got.active)
    # phase 0 is refit_exposures on the sub-catalogue, bit for bit
    H, err, nit, conv = tgm.sub_refit(X, W, C, FIXED)
    assert np.array_equal(got.dense_exposures, H) and np.array_equal(got.dense_errors, err)
    assert np.array_equal(got.dense_n_iterations, nit) and np.array_equal(got.dense_converged, conv)
    dH, dF = mref.deviations(got, ld, scale, rows)
    print(f"masks K={K} V={V}: isolated {ok.sum()} of {ok.size}, trials {got.n_trials.min()}..{got.n_trials.max()}, threshold margin {margin:.3g}, "
          f"u margin {umargin:.3g}, host spread H {h_spread:.3g} f {f_spread:.3g}, device H {dH:.3g} f {dF:.3g}, of the bounds "
          f"{dH / (16 * mref.H_SPREAD):.3g} {dF / (16 * mref.F_SPREAD):.3g}")
    assert dH <= 16 * mref.H_SPREAD
    assert dF <= 16 * mref.F_SPREAD


def phase_zero_reference(K, V):
    """(X, W, longdouble refit replica at the assignment's 20 steps, its row scales, float64 H spread, float64 f spread)."""
    X, W = tga.catalogue(N, K, V, 0)
    ld, h_spread = tgr.host_spread(X, W, **FIXED)
    scale = mref.row_scale(X, W, ld.exposures.astype(np.float64))
    perm = np.random.default_rng(mref.PERM_SEED).permutation(V)
    f_spread = max(float((np.abs(run.reconstruction_errors - ld.reconstruction_errors) / scale).max())
                   for run in (ref.refit(X, W, **FIXED), ref.refit(X, W, perm=perm, **FIXED)))
    return X, W, ld, scale, h_spread, f_spread


def test_assign_phase_zero_at_a_single_feature():
    """(15, 1): the dense solve of the plain call against the longdouble refit replica, and that of the masked call against
    ``sal.refit_exposures`` on every sample's sub-catalogue, bit for bit."""
    K, V = SHAPES[0]
    X, W, ld, scale, _, _ = phase_zero_reference(K, V)
    got = sal.assign_signatures(X, W, THR, **FIXED)
    dH = tgr.entry_dev(got.dense_exposures, ld.exposures)
    dF = float((np.abs(got.dense_errors - ld.reconstruction_errors.astype(np.float64)) / scale).max())
    print(f"assign phase 0 K={K} V={V}: device H {dH:.3g} f {dF:.3g}, of the bounds {dH / (16 * mref.H_SPREAD):.3g} {dF / (16 * mref.F_SPREAD):.3g}")
    assert dH <= 16 * mref.H_SPREAD and dF <= 16 * mref.F_SPREAD
    assert np.array_equal(got.dense_n_iterations, np.full(N, 20))
    C, _ = mref.case_sets(N, K, 0, "edge")
    masked = sal.assign_signatures(X, W, THR, candidates=C, readd=True, **FIXED)
    H, err, nit, conv = tgm.sub_refit(X, W, C, FIXED)
    assert np.array_equal(masked.dense_exposures, H) and np.array_equal(masked.dense_errors, err)
    assert np.array_equal(masked.dense_n_iterations, nit) and np.array_equal(masked.dense_converged, conv)
    assert (masked.dense_exposures[~C] == 0.0).all() and (masked.dense_exposures[C] >= EPS).all()


# ---- 3. presence, power, profile

def solve(X, W, C):
    return sal.assign_signatures(X, W, candidates=C, required=C, **FIT)


@pytest.mark.parametrize("K,V", SHAPES + WORD_EDGES)
def test_presence_fits_against_the_replica(K, V):
    """The observed statistic, the alternative and the null errors and both exposures at 20-step solves, with the bounds of
    ``test_gpu_profile.test_the_frozen_entry_and_the_replica``."""
    X, W, test, C = pair_case(K, V)
    want = pair_replica(K, V)
    got = sal.signature_presence_test(X, W, test, n_draws=1, seed=SEED, candidates=C, **STEPS)
    t = want.tested
    assert np.array_equal(got.tested, t) and t[:5].all() and not t[5:9, 0].any() and t[5:9, 1].all() and not t[9].any() and not t[10].any()
    assert np.array_equal(got.n_iterations[t], np.full((int(t.sum()), 2), 20))
    rows = np.flatnonzero(t.any(axis=1))
    scale = mref.row_scale(X[rows], W, want.exposures[rows])
    worst_h = float((np.abs(got.exposures[rows] - want.exposures[rows]) / np.maximum(want.exposures[rows], EPS))[C[rows]].max())
    worst_f = float((np.abs(got.reconstruction_errors[rows] - want.reconstruction_errors[rows]) / scale).max())
    assert (got.exposures[rows][~C[rows]] == 0.0).all()
    worst_g = 0.0
    for j, s in enumerate(test):
        rows = np.flatnonzero(t[:, j])
        free = C[rows].copy()
        free[:, s] = False
        H0, Hw = got.null_exposures[rows, j], want.profile_exposures[rows, j, 0]
        assert (H0[~free] == 0.0).all()
        scale = mref.row_scale(X[rows], W, Hw)
        worst_h = max(worst_h, float((np.abs(H0 - Hw) / np.maximum(Hw, EPS))[free].max()))
        worst_f = max(worst_f, float((np.abs(got.null_errors[rows, j] - want.errors[rows, j, 0]) / scale).max()))
        worst_g = max(worst_g, float((np.abs(got.statistic[rows, j] - want.profile[rows, j, 0]) / scale).max()))
    print(f"presence K={K} V={V}: |dH| / H {worst_h:.3g}, |df| / scale {worst_f:.3g}, |dg| / scale {worst_g:.3g}, of the bounds "
          f"{worst_h / (16 * mref.H_SPREAD):.3g} {worst_f / (16 * mref.F_SPREAD):.3g} {worst_g / (32 * mref.F_SPREAD):.3g}")
    assert worst_h <= 16 * mref.H_SPREAD
    assert worst_f <= 16 * mref.F_SPREAD
    assert worst_g <= 2 * 16 * mref.F_SPREAD


@functools.lru_cache(maxsize=None)
def power_run(K, V):
    X, W, test, C = pair_case(K, V)
    return sal.signature_power(X, W, test, shares=SHARES, n_draws=B, n_alt_draws=A, alpha=ALPHA, seed=SEED, candidates=C, keep_draws=True, **FIT)


@pytest.mark.parametrize("K,V", SHAPES + WORD_EDGES)
def test_presence_draws_equal_the_replica(K, V):
    """The draw is integer arithmetic after the weights: from the device's own null exposures, bit for bit."""
    X, W, test, C = pair_case(K, V)
    res = power_run(K, V).presence
    want = presence_ref.draws_from(res.null_exposures, W, X.sum(axis=1), test, res.tested, B, SEED)
    assert np.array_equal(res.draws, want)
    assert np.array_equal(res.draws.sum(axis=3), np.where(res.tested, X.sum(axis=1)[:, None], 0.0)[None].repeat(B, axis=0))
    if V > 1:  # (with one feature every draw is the row's total, and every solve sits at its fixed point after one step)
        assert not np.array_equal(res.draws[0, 4, 0], res.draws[0, 4, 1]) and not np.array_equal(res.draws[0, 4, 0], res.draws[1, 4, 0])
        assert 1 < np.unique(res.n_iterations[res.tested]).size  # problems of one tile stop at different tests
    once = sal.signature_presence_test(X, W, test, n_draws=B, seed=SEED, candidates=C, keep_draws=True, **FIT)
    for name in ("statistic", "n_exceed", "null_exposures", "null_errors", "null_statistics", "n_iterations", "draws"):
        assert np.array_equal(getattr(once, name), getattr(res, name), equal_nan=True), name


@pytest.mark.parametrize("K,V", SHAPES + WORD_EDGES)
def test_power_detections_are_the_presence_test_on_the_same_draws(K, V):
    X, W, test, C = pair_case(K, V)
    res = power_run(K, V)
    tested = res.presence.tested
    want = power_ref.draws_from(res.planted_exposures, W, X.sum(axis=1), test, tested, A, SEED)
    assert np.array_equal(res.alt_draws, want)
    for j, s in enumerate(test):
        rows = np.flatnonzero(tested[:, j])
        C0 = C[rows].copy()
        C0[:, s] = False
        for l in range(len(SHARES)):
            for a in range(A):
                drawn = res.alt_draws[l, a, rows, j]
                alt, null = solve(drawn, W, C[rows]), solve(drawn, W, C0)
                assert np.array_equal(res.alt_statistics[l, a, rows, j], null.reconstruction_errors - alt.reconstruction_errors), (s, l, a)
    e, n_detected, _ = power_ref.reduce_alt(res.presence.null_statistics, res.alt_statistics, power_ref.max_exceed(ALPHA, B))
    assert np.array_equal(res.alt_n_exceed, e) and np.array_equal(res.n_detected, n_detected)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res.n_detected[:, tested], ((1 + res.alt_n_exceed) / (B + 1) <= ALPHA).sum(axis=1)[:, tested])


@pytest.mark.parametrize("K,V", SHAPES + WORD_EDGES)
def test_profile_frozen_solves_against_the_replica(K, V, monkeypatch):
    """``test_gpu_profile.test_the_frozen_entry_and_the_replica`` on the inputs of this file."""
    monkeypatch.setattr(tgprof, "case", pair_case)
    tgprof.test_the_frozen_entry_and_the_replica(K, V)


# ---- 4. change, sigchange: ``_change_ref.gpu_case`` builds any shape, with the candidate-word edge in every set of a shape that
# is not one of its file's own; B = 3 draws, and every function below reads the one call per shape that ``run_of`` keeps

@pytest.mark.parametrize("K,V", SHAPES + WORD_EDGES)
def test_exposure_change_against_the_replica(K, V):
    """tests/test_gpu_change.py at the shape: the null divergences within 16 x ``_change_ref.G_SPREAD`` of longdouble, the draws
    equal to the replica's, the null statistics within their stated tolerance of the procedure on the kept draws; and the three
    fits against the masked solves, the untested pairs and the reduction."""
    C = tgch.ref.gpu_case(K, V)[3]
    assert C[:, [1, K - 1, 32 * ((K - 1) // 32)]][np.arange(N) != 9].all() and C[9].sum() == 1
    tgch.test_untested_pairs_and_shapes(K, V)
    tgch.test_observed_fits_are_the_three_masked_solves(K, V)
    tgch.test_statistic_and_null_divergences(K, V)
    tgch.test_draws_equal_the_replica(K, V)
    tgch.test_null_statistics_are_the_procedure_on_the_kept_draws(K, V)
    tgch.test_reduction(K, V)


@pytest.mark.parametrize("K,V", SHAPES + WORD_EDGES)
def test_signature_change_against_the_replica(K, V):
    """tests/test_gpu_sigchange.py at the shape, every solve 40 steps long: the tied solve within 16 x ``_sigchange_ref.H_SPREAD``
    / ``F_SPREAD`` of longdouble and the tie itself, the draws equal to the replica's, the null statistics within their stated
    tolerance of the procedure on the kept draws; and the free fits against the masked solves, and the reduction.  The tested
    signatures are 0, 32 floor((K - 1) / 32) and K - 1."""
    *_, test, res = tgsc.run_of(K, V)
    assert test[0] == 0 and test[-1] == K - 1 and 32 * ((K - 1) // 32) in test and res.test == test
    assert np.array_equal(res.tested, tgsc.ref.tested_problems(*tgsc.ref.gpu_case(K, V)[:2], res.candidates, test))
    tgsc.test_free_fits_are_the_two_masked_solves(K, V, "fixed")
    tgsc.test_tied_solve_against_the_longdouble_replica(K, V)
    tgsc.test_draws_equal_the_replica(K, V)
    tgsc.test_null_statistics_are_the_procedure_on_the_kept_draws(K, V)
    tgsc.test_reduction(K, V)


# ---- 5. covariance

@pytest.mark.parametrize("information", tgc.INFORMATION)
@pytest.mark.parametrize("K,V", SHAPES)
def test_covariance_against_the_extended_reference(K, V, information):
    X, W, H, active = cov_case(K, V)
    res = sal.exposure_covariance(X, W, H, active=active, information=information, return_correlation=True)
    tgc.check(res, cov_reference(K, V, information), COV_MEASURED[K, V, information], f"covariance K={K} V={V} {information}")
    assert res.correlation.shape == (N, K, K)


# ---- 6. independence at the edges

REFIT_NAMES = ("exposures", "reconstruction_errors", "n_iterations", "converged")
PRESENCE_NAMES = ("tested", "statistic", "exposures", "reconstruction_errors", "null_exposures", "null_errors", "n_iterations", "converged")


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("K,V", ONE_PER_KT)
def test_row_subsets_give_the_same_bits(K, V, n):
    rows = subset_rows(n)
    X, W = refit_case(K, V)
    full, part = sal.refit_exposures(X, W, **CONVERGING), sal.refit_exposures(X[rows], W, **CONVERGING)
    for name in REFIT_NAMES:
        assert np.array_equal(getattr(part, name), getattr(full, name)[rows]), name
    X, W, kw = mref.case_inputs(*masked_case(K, V))
    full = sal.assign_signatures(X, W, **kw, **CONVERGING)
    part = sal.assign_signatures(X[rows], W, **dict(kw, candidates=kw["candidates"][rows]), **CONVERGING)
    tgm.same(part, full, tgm.NAMES + tgm.READD, rows)
    if V > 1:
        assert 1 < np.unique(full.n_iterations).size and 1 < np.unique(full.n_trials).size
    # the presence test's fits do not see the sample index (its draws do)
    X, W, test, C = pair_case(K, V)
    full = sal.signature_presence_test(X, W, test, n_draws=1, seed=SEED, candidates=C, **FIT)
    part = sal.signature_presence_test(X[rows], W, test, n_draws=1, seed=SEED, candidates=C[rows], **FIT)
    for name in PRESENCE_NAMES:
        assert np.array_equal(getattr(part, name), getattr(full, name)[rows], equal_nan=True), name


# ---- 7. pads never leak

def embedded(a, extra=5):
    """`a` as a view of a wider array whose other columns hold NaN."""
    wide = np.full((a.shape[0], a.shape[1] + extra), np.nan)
    wide[:, 2:2 + a.shape[1]] = a
    return wide[:, 2:2 + a.shape[1]]


@pytest.mark.parametrize("K,V", PAD_SHAPES)
def test_columns_outside_the_views_never_leak(K, V):
    """Counts and signatures cut out of wider arrays whose other columns hold NaN: every output of the refit and of the assignment
    has the bits of the call on the arrays themselves.

    The other half of the pad check -- all-zero features appended to both the counts and the signatures -- has no output to
    compare: the contract clips a zero count to EPSILON and the appended signature column makes (h W)_v = 0 there, so the step's
    x / (h W) is infinite and its product with the zero signature entry NaN.  tests/test_family_edges_host.py shows it on the
    replica (every exposure and every objective of the widened problem is NaN), so the widened call is not a no-op of the
    contract and nothing of it is asserted."""
    X, W = refit_case(K, V)
    Xv, Wv = embedded(X), embedded(W)
    assert not Xv.flags.c_contiguous and np.array_equal(Xv, X) and np.array_equal(Wv, W)
    narrow, wide = sal.refit_exposures(X, W, **CONVERGING), sal.refit_exposures(Xv, Wv, **CONVERGING)
    for name in REFIT_NAMES:
        assert np.array_equal(getattr(wide, name), getattr(narrow, name)), name
    X, W, kw = mref.case_inputs(*masked_case(K, V))
    narrow = sal.assign_signatures(X, W, **kw, **FIXED)
    wide = sal.assign_signatures(embedded(X), embedded(W), **kw, **FIXED)
    tgm.same(wide, narrow, tgm.NAMES + tgm.READD)
