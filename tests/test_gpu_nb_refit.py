"""``sal.nb_refit_exposures`` and ``sal.estimate_dispersion`` on the device against the host replica (tests/_nb_ref.py),
DESIGN.md section 23.

No tolerance is tuned on the device.  The constants of tests/_nb_ref.py are float64-against-longdouble spreads measured on the
CPU on this file's inputs (tests/test_nb_ref_host.py asserts that they bound what it measures); the device -- a third summation
order, the MFMA's -- gets 16 x them, the family's margin.  H is compared entry by entry as |dH| / max(H_ref, EPSILON), a
divergence as |d| / objective_scale (the magnitudes of its terms).  Every figure is printed before it is asserted.
"""

import functools

import numpy as np
import pytest

import _nb_ref as ref
import salamander_amd as sal

pytestmark = pytest.mark.gpu

EPS = ref.EPSILON
H_TOL = ref.MARGIN * ref.H_SPREAD
D_TOL = ref.MARGIN * ref.D_SPREAD
G = ref.MARGIN * ref.G_RAW
FIELDS = ("exposures", "reconstruction_errors", "n_iterations", "converged", "log_likelihood", "dispersion")


@pytest.mark.parametrize("K,V", ref.FIXED_CASES)
def test_fixed_steps_entry_by_entry(K, V):
    X, W, alpha, kw = ref.fixed_case(K, V)
    N = X.shape[0]
    ld = ref.nb_refit(X, W, alpha, dtype=np.longdouble, **kw)
    got = sal.nb_refit_exposures(X, W, alpha, **kw)
    dev = ref.entry_dev(got.exposures, ld.exposures)
    derr = ref.objective_dev(got.reconstruction_errors, ld)
    print(f"fixed K={K} V={V}: H device {dev:.3g} tol {H_TOL:.3g}; divergence device {derr:.3g} tol {D_TOL:.3g}")
    assert np.isfinite(got.exposures).all() and got.exposures.shape == (N, K) and got.exposures.min() >= EPS
    assert dev <= H_TOL
    assert derr <= D_TOL
    assert np.array_equal(got.n_iterations, np.full(N, ref.FIXED_T))
    assert np.array_equal(got.dispersion, alpha)
    assert np.array_equal(got.log_likelihood, -got.reconstruction_errors + ref.constant(X, alpha))


@pytest.mark.parametrize("N,K", ref.CONVERGENCE_CASES)
def test_default_stopping_of_every_problem(N, K):
    X, W, alpha = ref.convergence_case(N, K)
    kw = ref.CONVERGENCE_KW
    got = sal.nb_refit_exposures(X, W, alpha, **kw)
    nit = got.n_iterations.astype(np.int64)
    own = ref.nb_refit(X, W, alpha, **kw)
    last = int(max(nit.max(), own.n_iterations.max()))
    free = ref.free_runs(X, W, alpha, last)
    g_raw, _ = ref.change_deviation(free, last)
    ld = free["ld"]
    tests = ld.tests
    eligible = tests >= kw["min_iterations"]
    same = int((nit == own.n_iterations).sum())
    print(f"stopping N={N} K={K}: iterations {nit.min()}..{np.median(nit):.0f}..{nit.max()}, equal to the replica's {same}/{N}, capped {int((~got.converged).sum())}, "
          f"g_raw {g_raw:.3g} (recorded {ref.G_RAW:.3g})")
    assert g_raw <= ref.G_RAW
    assert np.all(got.converged[nit < kw["max_iterations"]])  # (the cap is a test iteration here: the loop below covers nit == max_iterations)
    assert (~got.converged).any() and got.converged.any()  # (the problems at alpha = 0.5 converge slowly: some hit the cap)
    for p in range(N):  # every problem, near-ties included: where the device's stop is not the replica's, the longdouble sequence accepts it
        if got.converged[p]:
            i = int(np.flatnonzero(tests == nit[p])[0])
            assert nit[p] >= kw["min_iterations"] and nit[p] % kw["conv_test_freq"] == 0
            assert ld.changes[i, p] < kw["tol"] * (1 + G), (p, nit[p], ld.changes[i, p])
        else:
            assert nit[p] == kw["max_iterations"]
            i = len(tests)
        earlier = eligible & (np.arange(len(tests)) < i)
        assert np.all(ld.changes[earlier, p] >= kw["tol"] * (1 - G)), (p, nit[p])
    forced, spread = ref.schedule_spread(X, W, alpha, nit)
    dev = ref.entry_dev(got.exposures, forced.exposures)
    print(f"   H at the device's schedule: host spread {spread:.3g} device {dev:.3g} tol {ref.MARGIN * spread:.3g}")
    assert dev <= ref.MARGIN * spread


def test_converged_is_false_exactly_where_max_iterations_was_hit():
    X, W, alpha = ref.convergence_case(40, 8)
    kw = dict(min_iterations=20, max_iterations=55, conv_test_freq=10, tol=1e-3)  # (55 is no test iteration)
    got = sal.nb_refit_exposures(X, W, alpha, **kw)
    own = ref.nb_refit(X, W, alpha, **kw)
    print(f"cap: device iterations {np.unique(got.n_iterations)}, capped {int((~got.converged).sum())}; replica's equal at {int((got.n_iterations == own.n_iterations).sum())}/40")
    assert np.array_equal(~got.converged, got.n_iterations == 55)
    assert (~got.converged).any() and got.converged.any()
    assert np.all(got.n_iterations[got.converged] % 10 == 0) and np.all(got.n_iterations[got.converged] >= 20)
    # tol = 1e-3 against a deviation of the relative change of at most G_RAW x tol: no near-tie on these inputs
    assert np.array_equal(got.n_iterations, own.n_iterations) and np.array_equal(got.converged, own.converged)
    forced = ref.nb_refit(X, W, alpha, dtype=np.longdouble, schedule=own.n_iterations, **kw)
    assert ref.entry_dev(got.exposures, forced.exposures) <= H_TOL


@functools.lru_cache(maxsize=None)
def _independence_run():
    X, W = ref.catalogue(100, 6, seed=4)
    alpha = ref.mixed_alpha(100)
    kw = dict(min_iterations=30, max_iterations=200, conv_test_freq=10, tol=1e-5)
    return X, W, alpha, kw, sal.nb_refit_exposures(X, W, alpha, **kw)


@pytest.mark.parametrize("N", [1, 17])
def test_row_subsets_give_the_same_bits(N):
    X, W, alpha, kw, full = _independence_run()
    rows = np.random.default_rng(N).permutation(100)[:N]
    part = sal.nb_refit_exposures(X[rows], W, alpha[rows], **kw)
    for name in FIELDS:
        assert np.array_equal(getattr(part, name), getattr(full, name)[rows]), name
    assert 1 < np.unique(full.n_iterations).size


def test_permutation_scalar_dispersion_and_views_give_the_same_bits():
    X, W, alpha, kw, full = _independence_run()
    perm = np.random.default_rng(3).permutation(100)
    moved = sal.nb_refit_exposures(X[perm], W, alpha[perm], **kw)
    for name in FIELDS:
        assert np.array_equal(getattr(moved, name), getattr(full, name)[perm]), name
    scalar = sal.nb_refit_exposures(X, W, 20.0, **kw)
    array = sal.nb_refit_exposures(X, W, np.full(100, 20.0), **kw)
    for name in FIELDS:
        assert np.array_equal(getattr(scalar, name), getattr(array, name)), name
    twenty = alpha == 20.0
    assert np.array_equal(scalar.exposures[twenty], full.exposures[twenty])
    # inputs cut out of wider NaN-filled arrays
    wide_x = np.full((104, 120), np.nan)
    wide_x[2:102, 7:103] = X
    wide_w = np.full((10, 120), np.nan)
    wide_w[1:7, 20:116] = W
    wide_a = np.full(300, np.nan)
    wide_a[5:205:2] = alpha
    cut = sal.nb_refit_exposures(wide_x[2:102, 7:103], wide_w[1:7, 20:116], wide_a[5:205:2], **kw)
    for name in FIELDS:
        assert np.array_equal(getattr(cut, name), getattr(full, name)), name


def test_a_problem_of_the_dispersion_list_is_the_same_problem_alone():
    X, W = ref.catalogue(21, 5, seed=8)
    kw = dict(min_iterations=30, max_iterations=200, conv_test_freq=10, tol=1e-5)
    grid = np.array([0.7, 20.0, 3e3, 1e6])
    est = sal.estimate_dispersion(X, W, grid=grid, **kw)
    assert est.profile.shape == (4, 21) and est.exposures.shape == (4, 21, 5)
    for a, n in ((0, 0), (1, 20), (2, 7), (3, 13)):
        one = sal.nb_refit_exposures(X[n:n + 1], W, grid[a], **kw)
        assert np.array_equal(est.exposures[a, n], one.exposures[0]) and est.divergence[a, n] == one.reconstruction_errors[0]
        assert est.profile[a, n] == one.log_likelihood[0] and est.n_iterations[a, n] == one.n_iterations[0] and est.converged[a, n] == one.converged[0]
    whole = sal.nb_refit_exposures(X, W, grid[1], **kw)
    assert np.array_equal(est.profile[1], whole.log_likelihood)


def test_exact_properties_of_the_resamples():
    X, W = ref.catalogue(37, 5, seed=11)
    alpha = ref.mixed_alpha(37)
    kw = dict(min_iterations=50, max_iterations=300, conv_test_freq=10, tol=1e-6)
    qs = (0.025, 0.25, 0.5, 0.9, 0.975)
    r8 = sal.nb_refit_exposures(X, W, alpha, n_resamples=8, resample_seed=5, quantiles=qs, keep_resamples=True, **kw)
    r4 = sal.nb_refit_exposures(X, W, alpha, n_resamples=4, resample_seed=5, quantiles=qs, keep_resamples=True, **kw)
    small = sal.nb_refit_exposures(X, W, alpha, n_resamples=8, resample_seed=5, quantiles=qs, keep_resamples=True, chunk_bytes=3 * 37 * 96 * 8, **kw)
    assert r8.timings["n_chunks"] == 1 and small.timings["n_chunks"] == 3
    drawn = sal.resample_counts(X, 8, 5)
    for r in range(8):
        one = sal.nb_refit_exposures(drawn[r], W, alpha, **kw)  # a resample of sample n carries sample n's dispersion
        assert np.array_equal(r8.exposures_resampled[r], one.exposures), r
        assert np.array_equal(r8.n_iterations_resampled[r], one.n_iterations) and np.array_equal(r8.reconstruction_errors_resampled[r], one.reconstruction_errors)
    assert np.array_equal(r4.exposures_resampled, r8.exposures_resampled[:4])
    plain = sal.nb_refit_exposures(X, W, alpha, **kw)
    for name in ("exposures", "reconstruction_errors", "n_iterations", "converged", "log_likelihood"):
        assert np.array_equal(getattr(r8, name), getattr(plain, name)), name
    for name in ("exposures", "reconstruction_errors", "n_iterations", "converged", "exposures_resampled", "exposures_mean", "exposures_quantiles",
                 "n_iterations_resampled", "reconstruction_errors_resampled"):
        assert np.array_equal(getattr(small, name), getattr(r8, name)), name
    for res, R in ((r8, 8), (r4, 4)):
        total = np.zeros_like(res.exposures)
        for r in range(R):
            total = total + res.exposures_resampled[r]
        assert np.array_equal(res.exposures_mean, total / R)
        for i, q in enumerate(qs):
            assert np.array_equal(res.exposures_quantiles[i], np.quantile(res.exposures_resampled, q, axis=0, method="lower" if q <= 0.5 else "higher"))
    assert sal.nb_refit_exposures(X, W, alpha, n_resamples=2, **kw).exposures_resampled is None
    with pytest.raises(ValueError):
        sal.nb_refit_exposures(X, W, alpha, n_resamples=1025, **kw)


def test_the_c_entry_point_refuses_what_python_refuses():
    from salamander_amd import _lib

    lib = _lib.load_with_device()
    X, W = ref.catalogue(5, 2, seed=1)
    H, err = np.empty((5, 2)), np.empty(5)
    nit, conv = np.empty(5, dtype=np.int32), np.empty(5, dtype=np.int32)
    p = _lib.pointer
    for bad, R in ((0.0, 0), (np.nan, 0), (np.inf, 0), (2e6, 0), (-1.0, 0), (20.0, 1025)):
        alpha = np.full(5, 20.0)
        alpha[3] = bad
        status = lib.salnmf_nb_refit_exposures(0, p(X), 5, 96, p(W), 2, p(alpha), R, 0, 0, None, 10, 20, 10, 1e-7, 0, p(H), p(err), p(nit), p(conv),
                                               None, None, None, None, None, None)
        assert status == 1, (bad, R)


@pytest.mark.parametrize("poisson", [False, True])
def test_estimate_dispersion_against_the_replica(poisson):
    """The two inputs of the host recovery test.  A profile entry is -divergence + c with the same c on both sides, and both sides
    stop where a test's relative change is below tol: a stop one test apart moves the divergence by less than tol (1 + G) of
    itself, so 2 tol of the divergence is allowed on top of 16 x the recorded objective spread."""
    X, W = ref.recovery_data(poisson)
    want_profile, want_pll, fit = ref.dispersion_profile(X, W, ref.GRID)
    est = sal.estimate_dispersion(X, W)
    assert np.array_equal(est.grid, ref.GRID)
    A, N = want_profile.shape
    div = np.asarray(fit.reconstruction_errors, dtype=np.float64).reshape(A, N)
    scale = ref.objective_scale(fit.x, fit.W, fit.exposures, fit.alpha.reshape(-1, 1)).reshape(A, N)
    allowed = 2 * ref.CONVERGENCE_KW["tol"] * np.abs(div) + D_TOL * scale
    worst = float((np.abs(est.profile - want_profile) / allowed).max())
    same = int((est.n_iterations == fit.n_iterations.reshape(A, N)).sum())
    print(f"dispersion poisson={poisson}: profile deviation {worst:.3g} of the allowed; stops equal to the replica's {same}/{A * N}; "
          f"dispersion {est.dispersion:.4g}, lr {est.lr_statistic:.5g}")
    assert worst <= 1.0
    d, edge, lr = ref.select(ref.GRID, want_profile, want_pll)
    assert est.dispersion == d and bool(est.at_upper_edge) == bool(edge) == poisson
    assert abs(est.lr_statistic - lr) <= 2 * (allowed.sum(axis=1).max() + 2 * ref.CONVERGENCE_KW["tol"] * np.abs(want_pll).sum())
    pois = sal.refit_exposures(X, W)
    assert np.array_equal(est.poisson_log_likelihood, -pois.reconstruction_errors + ref.poisson_constant(X))
    ds, es, lrs = (sal.estimate_dispersion(X, W, per_sample=True).__dict__[k] for k in ("dispersion", "at_upper_edge", "lr_statistic"))
    assert ds.shape == (N,) and np.array_equal(ds, ref.GRID[np.argmax(est.profile, axis=0)]) and np.array_equal(es, ds == ref.GRID[-1])
    assert np.array_equal(lrs, 2.0 * (est.profile.max(axis=0) - est.poisson_log_likelihood))
