"""``sal.assign_signatures`` on the device against the host replica (tests/_assign_ref.py), DESIGN.md section 14.

Discrete decisions are compared exactly, and only where the CPU shows them isolated: the float64 replica in two feature
orders and the longdouble replica agree on every choice, every threshold comparison clears the threshold by
1e-6 max(1, |threshold|), and every chosen candidate is bit-equal to EPSILON or a relative 1e-6 below the runner-up.
Values get a tolerance that is not tuned on the device: the spread of the two float64 feature orders about the longdouble
replica, measured here on each case's own inputs, times 16 (the device is one more summation order of the same sums).  The
recorded constants are the largest spreads over this file's cases; each test asserts its own measurement stays within them.
"""

import functools
import os

import numpy as np
import pytest

import _assign_ref as aref
import _refit_ref as ref
import salamander_amd as sal

pytestmark = pytest.mark.gpu

EPS = ref.EPSILON
THR = 1.92
FIXED = dict(min_iterations=20, max_iterations=20, conv_test_freq=5)  # every solve is 20 steps long
H_SPREAD = 4.7e-15  # measured 4.62e-15 (P = 17, K = 16): largest |dH| / max(H_ld, EPS) on the support, float64 replica (two feature orders) against longdouble
F_SPREAD = 8.8e-16  # measured 8.70e-16 (P = 16, K = 17): largest |df| / scale and |d kl_increase| / scale, scale = sum_v |x log(x / wh)| + x + wh of the row
PERM_SEED = 7

# (P, K, V, seed): one tile, the tile boundary, a partial tile; K = 1, 2, 3, both sides of 16, 64, 96; a short feature axis
CASES = [(40, 1, 96, 0), (1, 2, 7, 0), (40, 3, 96, 0), (17, 16, 96, 0), (16, 17, 96, 0), (17, 64, 96, 0), (16, 96, 96, 0), (40, 3, 7, 0)]


def catalogue(P, K, V, seed):
    """Poisson counts whose last rows are near-empty (``zero_heavy``)."""
    return ref.poisson_catalogue(P, K, V=V, seed=seed, zero_heavy=min(3, P - 1))


@functools.lru_cache(maxsize=None)
def replicas(P, K, V, seed):
    """The case's inputs and its three host runs, computed once and shared by the tests that need them (never modified)."""
    X, W = catalogue(P, K, V, seed)
    perm = np.random.default_rng(PERM_SEED).permutation(V)
    runs = (aref.assign(X, W, THR, **FIXED), aref.assign(X, W, THR, perm=perm, **FIXED), aref.assign(X, W, THR, dtype=np.longdouble, **FIXED))
    return X, W, runs


def row_scale(X, W, H):
    x = np.maximum(X, EPS)
    wh = np.asarray(H, dtype=np.float64) @ W
    return (np.abs(x * np.log(x / wh)) + x + wh).sum(axis=1)


def deviations(got, ld, scale):
    """(H, f) deviations of a run from the longdouble replica `ld`, which has the same support."""
    H_ld = ld.exposures
    dH = float((np.abs(got.exposures - H_ld) / np.maximum(H_ld, EPS))[ld.active].max())
    df = float((np.abs(got.reconstruction_errors - ld.reconstruction_errors) / scale).max())
    tested = ~np.isnan(ld.kl_increase.astype(np.float64))
    dk = float((np.abs(got.kl_increase - ld.kl_increase) / scale[:, None])[tested].max(initial=0.0))
    return dH, max(df, dk)


def host_spread(X, W, runs):
    a, b, ld = runs
    scale = row_scale(X, W, ld.exposures)
    da, db = deviations(a, ld, scale), deviations(b, ld, scale)
    return scale, max(da[0], db[0]), max(da[1], db[1])


@pytest.mark.parametrize("P,K,V,seed", CASES)
def test_decisions_and_values_against_the_replica(P, K, V, seed):
    X, W, runs = replicas(P, K, V, seed)
    a, _, ld = runs
    ok, margin = aref.isolation(runs, THR)
    assert ok.all(), np.flatnonzero(~ok)  # every decision of every row is isolated, on the CPU
    scale, h_spread, f_spread = host_spread(X, W, runs)
    got = sal.assign_signatures(X, W, THR, **FIXED)
    # 1. decisions, exactly
    assert np.array_equal(got.active, a.active)
    assert np.array_equal(got.removal_round, a.removal_round)
    assert np.array_equal(got.n_trials, a.n_trials)
    assert np.array_equal(got.n_iterations, a.n_iterations) and np.array_equal(got.n_iterations, 20 * (got.n_trials + 1))
    # (a fixed-length solve may or may not pass its last tolerance test, so `converged` is not a decision of this test: a
    # problem without a trial made one solve, and its flag is that solve's)
    assert np.array_equal(got.converged[got.n_trials == 0], got.dense_converged[got.n_trials == 0])
    # 2. values
    assert np.array_equal(got.exposures == 0.0, ~got.active)
    assert np.array_equal(np.isnan(got.kl_increase), np.isnan(a.kl_increase))
    dH, dF = deviations(got, ld, scale)
    print(f"assign P={P} K={K} V={V}: trials {got.n_trials.min()}..{got.n_trials.max()}, threshold margin {margin:.3g}, "
          f"host spread H {h_spread:.3g} f {f_spread:.3g}, device H {dH:.3g} f {dF:.3g}")
    assert h_spread <= H_SPREAD and f_spread <= F_SPREAD
    assert dH <= 16 * H_SPREAD
    assert dF <= 16 * F_SPREAD


def test_problems_of_one_tile_finish_after_different_numbers_of_trials():
    X, W, runs = replicas(*CASES[3])
    got = sal.assign_signatures(X, W, THR, **FIXED)
    assert 1 < np.unique(got.n_trials[:16]).size and np.array_equal(got.n_trials, runs[0].n_trials)


NAMES = ("exposures", "active", "reconstruction_errors", "removal_round", "kl_increase", "n_trials", "n_iterations", "converged", "dense_exposures",
         "dense_errors", "dense_n_iterations", "dense_converged")
RESAMPLED = ("selection_frequency", "exposures_mean", "exposures_quantiles", "exposures_resampled")


def same(a, b, names=NAMES):
    for name in names:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name


@pytest.mark.parametrize("K,kw", [(5, FIXED), (17, FIXED), (96, FIXED), (6, dict(min_iterations=30, max_iterations=200, conv_test_freq=10, tol=1e-5))])
def test_phase_zero_is_refit_exposures_bit_for_bit(K, kw):
    X, W = catalogue(40, K, 96, seed=20 + K)
    got = sal.assign_signatures(X, W, THR, **kw)
    want = sal.refit_exposures(X, W, **kw)
    assert np.array_equal(got.dense_exposures, want.exposures) and np.array_equal(got.dense_errors, want.reconstruction_errors)
    assert np.array_equal(got.dense_n_iterations, want.n_iterations) and np.array_equal(got.dense_converged, want.converged)
    if kw is not FIXED:
        assert 1 < np.unique(want.n_iterations).size  # the problems of a tile leave phase 0 at different tests


@pytest.mark.parametrize("N", [1, 15, 16, 17])
def test_row_subsets_give_the_same_bits(N):
    X, W = catalogue(100, 6, 96, seed=4)
    kw = dict(min_iterations=30, max_iterations=200, conv_test_freq=10, tol=1e-5)
    full = sal.assign_signatures(X, W, THR, **kw)
    assert 1 < np.unique(full.n_iterations).size and 1 < np.unique(full.n_trials).size
    rows = np.random.default_rng(N).permutation(100)[:N]
    part = sal.assign_signatures(X[rows], W, THR, **kw)
    for name in NAMES:
        assert np.array_equal(getattr(part, name), getattr(full, name)[rows], equal_nan=True), name


def test_exact_properties_of_the_resamples():
    X, W = catalogue(37, 5, 96, seed=11)
    kw = dict(min_iterations=20, max_iterations=100, conv_test_freq=10, tol=1e-5)
    qs = (0.025, 0.25, 0.5, 0.9, 0.975)
    call = lambda R, **more: sal.assign_signatures(X, W, THR, n_resamples=R, resample_seed=5, quantiles=qs, keep_resamples=True, **kw, **more)  # noqa: E731
    r8, r4, again = call(8), call(4), call(8)
    small = call(8, chunk_bytes=3 * 37 * 96 * 8)
    assert r8.timings["n_chunks"] == 1 and small.timings["n_chunks"] == 3
    same(again, r8, NAMES + RESAMPLED)
    same(small, r8, NAMES + RESAMPLED)
    same(r4, r8)
    assert np.array_equal(r4.exposures_resampled, r8.exposures_resampled[:4])
    drawn = sal.resample_counts(X, 8, 5)
    for r in (0, 7):  # a resample's problems are those of a call on the drawn matrix
        assert np.array_equal(r8.exposures_resampled[r], sal.assign_signatures(drawn[r], W, THR, **kw).exposures), r
    for res, R in ((r8, 8), (r4, 4)):
        Hr = res.exposures_resampled
        assert (Hr == 0.0).any() and (Hr > 0.0).any()
        assert np.array_equal(res.selection_frequency, (Hr > 0).mean(axis=0))
        assert np.array_equal(res.selection_frequency * R, np.rint(res.selection_frequency * R))
        mean, quant = ref.reduce_resamples(Hr, qs)
        assert np.array_equal(res.exposures_mean, mean) and np.array_equal(res.exposures_quantiles, quant)
    none = sal.assign_signatures(X, W, THR, n_resamples=2, **kw)
    assert none.exposures_resampled is None and none.selection_frequency.shape == (37, 5)
    assert sal.assign_signatures(X, W, THR, **kw).selection_frequency is None


def test_convergence_mode_recovers_the_planted_supports():
    """Default stop rule on the planted catalogue (seed 0: the replica's decisions are isolated in 12 of 12 rows)."""
    X, W, planted = aref.planted_catalogue(seed=0)
    perm = np.random.default_rng(PERM_SEED).permutation(96)
    runs = (aref.assign(X, W, THR), aref.assign(X, W, THR, perm=perm), aref.assign(X, W, THR, dtype=np.longdouble))
    ok, margin = aref.isolation(runs, THR)
    assert (~ok).sum() <= 2
    got = sal.assign_signatures(X, W, THR)
    print(f"planted, defaults: isolated rows {ok.sum()} of 12, threshold margin {margin:.3g}, iterations {got.n_iterations.min()}..{got.n_iterations.max()}")
    assert (got.active | ~planted).all()
    assert np.array_equal(got.active[ok], runs[0].active[ok])
    assert np.array_equal(got.exposures == 0.0, ~got.active) and got.converged.all()


def test_pcawg_consensus_signatures_feed_the_assignment():
    import pandas as pd

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcawg_breast_sbs.csv")
    counts = pd.read_csv(path, index_col=0).T  # samples x 96
    adata = sal.AnnData(counts.values.astype(np.float64))
    adata.var_names = list(counts.columns)
    sweep = sal.models.KLNMFSweep(ns_signatures=[4], seeds=[0, 1, 2], stability=True, min_iterations=200, max_iterations=400)
    sweep.fit(adata)
    S = np.asarray(sweep.consensus_signatures_[0])
    res = sal.assign_signatures(adata, S, n_resamples=8, min_iterations=100, max_iterations=2000)
    N = adata.X.shape[0]
    assert res.exposures.shape == (N, 4) and res.active.any(axis=1).all()
    assert np.array_equal(res.exposures == 0.0, ~res.active)
    assert (res.reconstruction_errors - res.dense_errors <= THR * res.n_trials + 1e-9).all()  # every accepted removal cost at most THR
    assert ((0 <= res.selection_frequency) & (res.selection_frequency <= 1)).all()
