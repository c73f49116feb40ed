"""The sparse assignment's host side without a device: the replica (tests/_assign_ref.py) against the refit's replica, its
limits, planted recovery, and every argument ``sal.assign_signatures`` refuses before it touches a device."""

import numpy as np
import pytest

import _assign_ref as aref
import _refit_ref as ref
import salamander_amd as sal
from salamander_amd import assign as assign_mod


def test_phase_zero_is_the_refit_replica_exactly():
    X, W = ref.poisson_catalogue(20, 5, seed=2, zero_heavy=2)
    kw = dict(min_iterations=20, max_iterations=400, conv_test_freq=10, tol=1e-5)
    want = ref.refit(X, W, **kw)
    assert 1 < np.unique(want.n_iterations).size  # the rows leave phase 0 at different tests
    got = aref.assign(X, W, **kw).dense
    for name in ("exposures", "reconstruction_errors", "n_iterations", "converged"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


def test_threshold_limits_remove_nothing_and_all_but_one():
    X, W = ref.poisson_catalogue(9, 6, seed=4, zero_heavy=2)
    kw = dict(min_iterations=300, max_iterations=300, conv_test_freq=5)
    none = aref.assign(X, W, max_kl_increase=-1.0, **kw)
    # (a trial iterates on from where phase 0 stopped, so it can end below f -- but not by 1 once the 300 steps of phase 0 have
    # brought every row within 1 of its optimum; 20 steps do not)
    assert none.active.all() and np.array_equal(none.n_trials, np.full(9, 6)) and (none.removal_round == -1).all()
    assert np.array_equal(none.exposures, none.dense.exposures) and np.array_equal(none.reconstruction_errors, none.dense.reconstruction_errors)
    assert not np.isnan(none.kl_increase).any() and (none.exposures >= ref.EPSILON).all()
    one = aref.assign(X, W, max_kl_increase=1e300, **kw)
    assert np.array_equal(one.active.sum(axis=1), np.ones(9)) and np.array_equal(one.n_trials, np.full(9, 5))
    assert np.array_equal(np.sort(one.removal_round, axis=1), np.tile(np.arange(-1, 5), (9, 1)))
    assert np.array_equal(one.exposures == 0.0, ~one.active)
    assert np.array_equal(np.isnan(one.kl_increase), one.active)  # the survivor is never tried
    assert np.array_equal(one.n_iterations, np.full(9, 6 * 300))


def test_a_problem_does_not_depend_on_the_other_rows():
    X, W = ref.poisson_catalogue(14, 5, seed=6, zero_heavy=2)
    kw = dict(min_iterations=10, max_iterations=200, conv_test_freq=10, tol=1e-4)
    full = aref.assign(X, W, **kw)
    assert 1 < np.unique(full.n_iterations).size and 1 < np.unique(full.n_trials).size
    rows = np.array([3, 12, 0, 13])
    part = aref.assign(X[rows], W, **kw)
    for name in ("exposures", "active", "reconstruction_errors", "removal_round", "kl_increase", "n_trials", "n_iterations", "converged"):
        assert np.array_equal(getattr(part, name), getattr(full, name)[rows], equal_nan=True), name


def test_planted_supports_are_recovered():
    """Rows with 3 of 12 Dirichlet(0.15) signatures, 450-3 500 mutations, 200 fixed steps, threshold 1.92.  The replica keeps
    a superset of the planted support in 12 of 12 rows and exactly the planted support in 11 of 12 (seed 0, the committed
    one; seeds 0..11 of this generator all give 12 supersets and 9 to 12 exact rows, seed 5 the 9)."""
    X, W, planted = aref.planted_catalogue(seed=0)
    assert np.array_equal(planted.sum(axis=1), np.full(12, 3)) and 450 * 0.8 < X.sum(axis=1).min() and X.sum(axis=1).max() < 3500 * 1.2
    got = aref.assign(X, W, max_kl_increase=1.92, min_iterations=200, max_iterations=200, conv_test_freq=10)
    superset = (got.active | ~planted).all(axis=1)
    equal = (got.active == planted).all(axis=1)
    print(f"planted: superset in {superset.sum()} of 12 rows, equal in {equal.sum()} of 12")
    assert superset.all()
    assert equal.sum() >= 10


def test_refusals_come_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(assign_mod._lib, "load", no_device)
    X, W = ref.poisson_catalogue(4, 3, V=10, seed=0)
    bad = [(X, np.ones((97, 10))), (np.ones((3, 97)), np.ones((2, 97))), (X, np.ones((3, 9))), (X, np.zeros((0, 10))), (X, -W), (-X, W), (X[0], W),
           (X[:0], W)]
    for counts, sigs in bad:
        with pytest.raises(ValueError):
            sal.assign_signatures(counts, sigs)
    for kw in (dict(max_iterations=1005), dict(min_iterations=3, max_iterations=7, conv_test_freq=5), dict(max_kl_increase=float("inf")),
               dict(max_kl_increase=float("nan")), dict(max_kl_increase=-float("inf")), dict(max_kl_increase="1.92"), dict(n_resamples=1025),
               dict(n_resamples=-1), dict(conv_test_freq=0), dict(tol=-1.0), dict(min_iterations=20, max_iterations=10), dict(quantiles=(0.5, 1.5)),
               dict(chunk_bytes=0)):
        with pytest.raises(ValueError):
            sal.assign_signatures(X, W, **kw)
    with pytest.raises(ValueError, match="non-negative integer counts"):
        sal.assign_signatures(X + 0.5, W, n_resamples=2)
    for kw in (dict(max_iterations=7, conv_test_freq=5), dict(max_kl_increase=float("inf"))):
        with pytest.raises(ValueError):
            aref.assign(X, W, **kw)
    # a valid call gets as far as the library
    with pytest.raises(AssertionError, match="library was loaded"):
        sal.assign_signatures(X, W, max_kl_increase=0.0, max_iterations=1000)
