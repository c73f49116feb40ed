"""The refit's host side without a device: the replica (tests/_refit_ref.py) against the oracle, its independence of the
other rows, the quantile rule against NumPy's, and every argument ``sal.refit_exposures`` refuses before it touches a device."""

import numpy as np
import pytest

import _refit_ref as ref
import salamander_amd as sal
from oracle import klnmf_oracle as orc
from salamander_amd import refit as refit_mod


def test_one_step_is_the_oracles_update_H():
    X, W = ref.poisson_catalogue(40, 7, seed=1, zero_heavy=3)
    x = np.maximum(X, ref.EPSILON)
    h0 = ref.start(x, 7)
    want = orc.update_H(x.T, W.T, h0.T).T
    got = ref.refit(X, W, min_iterations=1, max_iterations=1).exposures
    # the same formula; the oracle contracts W @ H in the transposed orientation, so the sums may round differently
    assert np.abs(got - want).max() <= 64 * 2.0**-52 * np.abs(want).max()
    assert np.array_equal(got, ref.step(x, W, h0))
    # the objective is the per-sample divergence of the oracle on the clipped x
    kl = orc.samplewise_kl_divergence(x.T, W.T, got.T)
    scale = (np.abs(x * np.log(x / (got @ W))) + x + got @ W).sum(axis=1)
    assert np.all(np.abs(ref.objective(x, W, got) - kl) <= 256 * 2.0**-52 * scale)


def test_a_problem_does_not_depend_on_the_other_rows():
    X, W = ref.poisson_catalogue(30, 5, seed=2, zero_heavy=2)
    kw = dict(min_iterations=20, max_iterations=400, conv_test_freq=10, tol=1e-5)
    full = ref.refit(X, W, **kw)
    assert 1 < np.unique(full.n_iterations).size  # the rows stop at different tests: the latch is exercised
    rows = np.array([3, 28, 11, 29])
    part = ref.refit(X[rows], W, **kw)
    one = ref.refit(X[7:8], W, **kw)
    for name in ("exposures", "reconstruction_errors", "n_iterations", "converged"):
        assert np.array_equal(getattr(part, name), getattr(full, name)[rows]), name
        assert np.array_equal(getattr(one, name), getattr(full, name)[7:8]), name


def test_forced_schedule_and_free_run_agree_with_the_tested_run():
    X, W = ref.poisson_catalogue(12, 4, seed=3)
    kw = dict(min_iterations=20, max_iterations=300, conv_test_freq=10, tol=1e-5)
    full = ref.refit(X, W, **kw)
    forced = ref.refit(X, W, schedule=full.n_iterations, **kw)
    assert np.array_equal(forced.exposures, full.exposures) and np.array_equal(forced.reconstruction_errors, full.reconstruction_errors)
    free = ref.refit(X, W, free_run=True, **kw)
    for p in range(12):  # the first eligible test whose change is below tol is where the tested run stopped
        ok = np.flatnonzero((free.tests >= 20) & (free.changes[:, p] < 1e-5))
        assert (free.tests[ok[0]] if ok.size else 300) == full.n_iterations[p]
    ld = ref.refit(X, W, dtype=np.longdouble, **kw)
    assert np.abs(ld.exposures - full.exposures).max() < 1e-6 * np.abs(full.exposures).max()


@pytest.mark.parametrize("R", [1, 2, 5, 8, 41, 100, 101, 1000, 1024])
def test_quantile_indices_are_numpys_lower_and_higher(R):
    rng = np.random.default_rng(R)
    values = rng.normal(size=R)
    qs = np.array([0.0, 0.025, 0.05, 0.25, 0.5, 0.75, 0.9, 0.975, 1.0])
    idx = ref.quantile_indices(qs, R)
    assert np.array_equal(idx, refit_mod.quantile_indices(qs, R))
    srt = np.sort(values)
    for q, i in zip(qs, idx):
        want = np.quantile(values, q, method="lower" if q <= 0.5 else "higher")
        assert srt[i] == want, (R, q, i)
    mean, quant = ref.reduce_resamples(values.reshape(R, 1, 1), qs)
    assert np.array_equal(quant[:, 0, 0], srt[idx]) and abs(mean[0, 0] - values.mean()) < 1e-12


def test_refusals_come_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(refit_mod._lib, "load", no_device)
    X, W = ref.poisson_catalogue(4, 3, V=10, seed=0)
    bad = [
        (X, np.ones((97, 10))), (np.ones((3, 97)), np.ones((2, 97))), (X, np.ones((3, 9))), (X, np.zeros((0, 10))),
        (X, np.vstack([W[:2], np.zeros((1, 10))])), (X, -W), (X, np.where(W == W[0, 0], np.nan, W)), (-X, W), (np.full_like(X, np.inf), W),
        (X[0], W), (X[:0], W),
    ]
    for counts, sigs in bad:
        with pytest.raises(ValueError):
            sal.refit_exposures(counts, sigs)
    for kw in (dict(n_resamples=-1), dict(n_resamples=1025), dict(n_resamples=1.5), dict(resample_seed=-1), dict(min_iterations=5, max_iterations=4),
               dict(conv_test_freq=0), dict(tol=-1.0), dict(tol=float("nan")), dict(quantiles=(0.5, 1.5)), dict(quantiles=tuple([0.5] * 17)),
               dict(chunk_bytes=0)):
        with pytest.raises(ValueError):
            sal.refit_exposures(X, W, **kw)
    with pytest.raises(ValueError, match="non-negative integer counts"):
        sal.refit_exposures(X + 0.5, W, n_resamples=2)  # fractional counts are fine without resamples, refused with them
    a, s = sal.AnnData(X.copy()), sal.AnnData(W.copy())
    s.var_names = [f"other{v}" for v in range(10)]
    with pytest.raises(ValueError, match="features"):
        sal.refit_exposures(a, s)
    # a valid call gets as far as the library
    with pytest.raises(AssertionError, match="library was loaded"):
        sal.refit_exposures(X + 0.5, W)


def test_signatures_are_scaled_not_clipped():
    S = np.array([[0.0, 2.0, 2.0], [1.0, 0.0, 3.0]])
    W = refit_mod.normalize_signatures(S)
    assert np.array_equal(W, S / S.sum(axis=1, keepdims=True)) and (W == 0).sum() == 2
