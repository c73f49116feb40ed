"""The negative-binomial refit on the host: the replica's own properties, the yardsticks of tests/test_gpu_nb_refit.py measured
on the CPU on that file's inputs, the host-side arithmetic of ``salamander_amd/nb.py`` and every refusal.

No tolerance here comes from a device.  The spreads are those of the float64 replica in two feature orders against the
longdouble replica; the constants recorded in tests/_nb_ref.py (and in DESIGN.md) must bound them, so they cannot drift from the
inputs.
"""

import numpy as np
import pytest

import _nb_ref as ref
import salamander_amd as sal
from salamander_amd import _lib
from salamander_amd import nb as nb_mod

EPS = ref.EPSILON
U = 2.0**-52


@pytest.fixture
def no_device(monkeypatch):
    def refuse():
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "load_with_device", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


@pytest.mark.parametrize("alpha", ref.ALPHAS)
def test_the_objective_never_rises_beyond_rounding(alpha):
    """200 majorise-minimise steps, the objective after every one.  An evaluation's rounding is a few ulp of objective_scale (each
    term rounded once, x + alpha and p + alpha rounded before the second logarithm, a pairwise sum), so a rise between two
    evaluations is held to 4 ulp of it; measured: at most 0.26 ulp, at any alpha."""
    X, W = ref.catalogue(40, 3, 96, seed=99)
    f = ref.nb_refit(X, W, alpha, min_iterations=200, max_iterations=200, conv_test_freq=1, free_run=True)
    o = f.objectives
    assert o.shape == (201, 40) and np.all(o >= -4 * U * ref.objective_scale(f.x, f.W, f.exposures, f.alpha.reshape(-1, 1)))
    scale = ref.objective_scale(f.x, f.W, f.exposures, f.alpha.reshape(-1, 1))
    rise = float(((o[1:] - o[:-1]) / scale).max())
    print(f"alpha={alpha}: largest rise {rise / U:.3g} ulp of the scale; objective {o[0].max():.4g} -> {o[-1].max():.4g}")
    assert rise <= 4 * U
    assert np.all(o[-1] <= o[0])


def test_the_objective_tends_to_the_kl_divergence_and_vanishes_at_p_equal_x():
    import _refit_ref

    X, W = ref.catalogue(12, 3, 96, seed=5)
    x = np.maximum(X, EPS).astype(np.longdouble)
    h = ref.start(x, 3)
    Wl = W.astype(np.longdouble)
    kl = _refit_ref.objective(x, Wl, h)
    gaps = [float(np.abs(ref.objective(x, Wl, h, np.longdouble(a)) - kl).max() / kl.max()) for a in (1e6, 1e9, 1e12)]
    assert gaps[0] > gaps[1] > gaps[2] and gaps[2] < 1e-6
    # p = x: one signature equal to the row
    row = x[:1] / x[:1].sum()
    assert abs(float(ref.objective(x[:1], row, x[:1].sum(axis=1, keepdims=True), np.longdouble(20.0))[0])) < 1e-12


@pytest.mark.parametrize("alpha", [0.5, 20.0, 1e4])
def test_divergence_and_constant_give_the_negative_binomial_log_likelihood(alpha):
    """-divergence + c against sum_v scipy.stats.nbinom.logpmf on integer counts >= 1, both held to the longdouble value
    (lgamma differences as sums of logarithms).  Each of the eight terms per entry is rounded at a few ulp of its magnitude
    (gammaln's own error is a few ulp), so the bound is 8 ulp of the summed magnitudes; printed: what is measured."""
    from scipy.special import gammaln
    from scipy.stats import nbinom

    X, W = ref.catalogue(16, 4, 96, seed=21)
    X = np.maximum(X, 1.0)
    h = ref.nb_refit(X, W, alpha, min_iterations=50, max_iterations=50).exposures
    p = h @ W
    ours = -ref.objective(X, W, h, alpha) + ref.constant(X, alpha)
    assert np.array_equal(ref.constant(X, alpha), nb_mod.nb_constant(X, np.full(16, alpha)))
    scipy_ll = nbinom.logpmf(X, alpha, alpha / (alpha + p)).sum(axis=1)
    ld = ref.nbinom_logpmf_ld(X, alpha, p)
    xa = X + alpha
    mag = (gammaln(xa) + abs(gammaln(alpha)) + gammaln(X + 1.0) + np.abs(X * np.log(X)) + np.abs(xa * np.log(xa)) + abs(alpha * np.log(alpha))
           + np.abs(X * np.log(X / p)) + np.abs(xa * np.log(xa / (p + alpha)))).sum(axis=1)
    d_ours, d_scipy = float((np.abs(ours - ld) / mag).max()), float((np.abs(scipy_ll - ld) / mag).max())
    print(f"alpha={alpha}: ours {d_ours / U:.3g} ulp, scipy {d_scipy / U:.3g} ulp of the summed magnitudes; log-likelihoods {ld.min():.5g} .. {ld.max():.5g}")
    assert d_ours <= 8 * U and d_scipy <= 8 * U


@pytest.mark.parametrize("K,V", ref.FIXED_CASES)
def test_recorded_spreads_bound_the_fixed_step_cases(K, V):
    X, W, alpha, kw = ref.fixed_case(K, V)
    ld, h_spread, d_spread = ref.host_spread(X, W, alpha, **kw)
    print(f"K={K} V={V}: H spread {h_spread:.3g} (recorded {ref.H_SPREAD:.3g}), objective spread {d_spread:.3g} (recorded {ref.D_SPREAD:.3g})")
    assert h_spread <= ref.H_SPREAD and d_spread <= ref.D_SPREAD
    assert np.array_equal(ld.n_iterations, np.full(ref.FIXED_N, ref.FIXED_T))


@pytest.mark.parametrize("N,K", ref.CONVERGENCE_CASES)
def test_recorded_change_deviation_bounds_the_convergence_cases(N, K):
    X, W, alpha = ref.convergence_case(N, K)
    own = ref.nb_refit(X, W, alpha, **ref.CONVERGENCE_KW)
    last = int(own.n_iterations.max())
    g_raw, ld_stop = ref.change_deviation(ref.free_runs(X, W, alpha, last), last)
    print(f"N={N} K={K}: iterations {own.n_iterations.min()}..{last}, capped {int((~own.converged).sum())}, g_raw {g_raw:.3g} (recorded {ref.G_RAW:.3g})")
    assert g_raw <= ref.G_RAW
    assert np.all(own.converged | (own.n_iterations == ref.CONVERGENCE_KW["max_iterations"]))


def _profiles():
    out = {}
    for poisson in (False, True):
        X, W = ref.recovery_data(poisson)
        profile, pll, fit = ref.dispersion_profile(X, W, ref.GRID)
        out[poisson] = (X, W, profile, pll, fit)
    return out


@pytest.fixture(scope="module")
def profiles():
    return _profiles()


def test_dispersion_recovery(profiles):
    """Gamma-Poisson data with true alpha = 20 (seed ref.RECOVERY_SEED = 0, N = 64, K = 4, V = 96, mu = 2000), the replica run to the
    defaults' stop: the cohort argmax is a grid neighbour of 20; on Poisson data from the same means it is the last grid value."""
    X, W, profile, pll, fit = profiles[False]
    assert fit.converged.all()
    d, edge, lr = ref.select(ref.GRID, profile, pll)
    i = int(np.argmin(np.abs(np.log(ref.GRID / 20.0))))
    print(f"gamma-Poisson: argmax {d:.4g} (neighbours of 20: {ref.GRID[i - 1]:.4g}, {ref.GRID[i]:.4g}, {ref.GRID[i + 1]:.4g}), lr {lr:.5g}")
    assert d in (ref.GRID[i - 1], ref.GRID[i], ref.GRID[i + 1]) and not edge
    Xp, _, profile_p, pll_p, _ = profiles[True]
    dp, edge_p, lr_p = ref.select(ref.GRID, profile_p, pll_p)
    print(f"Poisson: argmax {dp:.4g}, lr {lr_p:.5g}")
    assert dp == ref.GRID[-1] and edge_p
    # the package's selection is the replica's
    for per_sample in (False, True):
        for prof, ll in ((profile, pll), (profile_p, pll_p)):
            got, want = nb_mod.select_dispersion(ref.GRID, prof, ll, per_sample), ref.select(ref.GRID, prof, ll, per_sample)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(nb_mod.poisson_constant(X), ref.poisson_constant(X))


def test_lr_statistic_is_not_negative_beyond_its_noise(profiles):
    """l_NB(alpha-hat) is the largest of the profile, so it is at least the NB log-likelihood at the LAST grid value evaluated at
    the Poisson fit's exposures, up to what the solver left undone: lr >= 2 (l_NB(grid[-1]; h_Poisson) - l_Poisson) - slack.  The
    first term is the real, small price of a finite top of the grid (of the order of sum_v [(x - p)^2 - x] / (2 alpha)); the slack
    is 2e-4 of the summed divergences: a stop at relative change < 1e-7 per test leaves at most 1e-4 of the objective if the
    last tests contract by a factor <= 0.999 each."""
    import _refit_ref

    for poisson in (True, False):
        X, W, profile, pll, _ = profiles[poisson]
        pois = _refit_ref.refit(X, W)
        top = ref.GRID[-1]
        at_poisson_fit = -ref.objective(np.maximum(X, EPS), W, pois.exposures, top) + ref.constant(X, top)
        slack = 2e-4 * np.abs(pois.reconstruction_errors)
        for per_sample in (False, True):
            _, _, lr = ref.select(ref.GRID, profile, pll, per_sample)
            floor = 2 * (at_poisson_fit - pll) - slack
            if not per_sample:
                floor = floor.sum()
            print(f"poisson={poisson} per_sample={per_sample}: lr min {np.min(lr):.5g}, floor at that entry {np.min(floor):.5g}")
            assert np.all(lr >= floor)
    assert np.min(ref.select(ref.GRID, *profiles[False][2:4], True)[2]) > -1.0 and ref.select(ref.GRID, *profiles[False][2:4])[2] > 100.0


def test_every_refusal_comes_before_the_device(no_device):
    X, W = ref.catalogue(6, 3, 96, seed=1)
    for bad in (0.0, -1.0, np.nan, np.inf, 1.0000001e6, [1.0] * 5, [1.0] * 7, np.ones((6, 1)), [1.0, 2.0, 3.0, 4.0, 5.0, -6.0], [1.0, 2.0, 3.0, 4.0, np.nan, 6.0], "x"):
        with pytest.raises(ValueError):
            sal.nb_refit_exposures(X, W, bad)
    Xf = X.copy()
    Xf[0, 0] += 0.5
    with pytest.raises(ValueError):
        sal.nb_refit_exposures(Xf, W, 20.0, n_resamples=4)
    with pytest.raises(ValueError):
        sal.nb_refit_exposures(X, W, 20.0, n_resamples=1025)
    with pytest.raises(ValueError):
        sal.nb_refit_exposures(X, W[:, :95], 20.0)
    with pytest.raises(ValueError):
        sal.nb_refit_exposures(X, W, 20.0, min_iterations=10, max_iterations=5)
    for grid in ([], [1.0, 1.0], [2.0, 1.0], [1.0, 3.0, 2.0], [0.0, 1.0], [1.0, np.inf], [1.0, 2e6], np.ones((2, 2)), [1.0, np.nan]):
        with pytest.raises(ValueError):
            sal.estimate_dispersion(X, W, grid=grid)
    with pytest.raises(ValueError):
        sal.estimate_dispersion(-X, W)
    # what passes the checks reaches the device (here: the fixture's refusal)
    with pytest.raises(AssertionError, match="the device was touched"):
        sal.nb_refit_exposures(X, W, 1e6)
    with pytest.raises(AssertionError, match="the device was touched"):
        sal.estimate_dispersion(Xf, W, grid=[1.0])


def test_public_names_and_result_fields():
    assert {"nb_refit_exposures", "NBRefitResult", "estimate_dispersion", "DispersionResult"} <= set(sal.__all__)
    assert sal.NBRefitResult is nb_mod.NBRefitResult and issubclass(sal.NBRefitResult, sal.RefitResult)
    assert "salnmf_nb_refit_exposures" in _lib.SIGNATURES
    doc = sal.estimate_dispersion.__doc__
    assert "No p-value" in doc and "Bias" in doc and "17.8" in doc
    assert np.array_equal(nb_mod.check_dispersion(3.0, 4), np.full(4, 3.0))
