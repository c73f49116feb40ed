"""``sal.nb_goodness_of_fit`` and ``sal.dispersion_test`` on the device: the observed and the null fits
against ``sal.nb_refit_exposures``, the draws against ``sal.draw_nb_counts``, the reduction against its stated rules -- every
comparison ``np.array_equal`` --, the calibration samples of tests/test_nbdraw_host.py, and the two dispersion calibrations on
the inputs the host replica was checked on."""

import numpy as np
import pytest

import _gof_ref as gof_ref
import _nb_ref as nb_ref
import _nbdraw_ref as ref
import salamander_amd as sal
from salamander_amd import _lib

pytestmark = pytest.mark.gpu

N = 40  # two full tiles of 16 problems and a partial one
FIT = dict(min_iterations=20, max_iterations=60, conv_test_freq=10, tol=1e-5)
FIT_NAMES = ("exposures", "reconstruction_errors", "n_iterations", "converged")
ALL_NAMES = FIT_NAMES + ("n_exceed", "p_value", "null_mean", "null_errors", "null_n_iterations", "draws", "log_likelihood")

_results = {}


def fitted(K):
    """One nb_goodness_of_fit call per K, shared by the tests that read it (none changes it)."""
    if K not in _results:
        X, W = nb_ref.catalogue(N, K, seed=40 + K)
        alpha = nb_ref.mixed_alpha(N)
        _results[K] = (X, W, alpha, sal.nb_goodness_of_fit(X, W, alpha, n_draws=5, seed=9, keep_draws=True, **FIT))
    return _results[K]


@pytest.mark.parametrize("K", [3, 17])
def test_observed_fit_is_the_nb_refit(K):
    X, W, alpha, res = fitted(K)
    want = sal.nb_refit_exposures(X, W, alpha, **FIT)
    for name in FIT_NAMES + ("log_likelihood", "dispersion"):
        assert np.array_equal(getattr(res, name), getattr(want, name)), name
    assert res.n_iterations.dtype == np.int32 and res.converged.dtype == bool


@pytest.mark.parametrize("K", [3, 17])
def test_null_fits_are_nb_refits_of_the_draws(K):
    X, W, alpha, res = fitted(K)
    assert res.draws.shape == (5, N, 96) and res.null_errors.shape == (5, N) and res.null_n_iterations.shape == (5, N)
    assert np.array_equal(res.draws, sal.draw_nb_counts(res.exposures, W, alpha, 5, 9))
    assert len(set(res.draws[:, 0].sum(axis=1))) > 1  # unconditional: a row's total varies
    for b in range(5):
        one = sal.nb_refit_exposures(res.draws[b], W, alpha, **FIT)
        assert np.array_equal(res.null_errors[b], one.reconstruction_errors), b
        assert np.array_equal(res.null_n_iterations[b], one.n_iterations), b


@pytest.mark.parametrize("K", [3, 17])
def test_reduction(K):
    X, W, alpha, res = fitted(K)
    assert res.n_exceed.dtype == np.int32
    assert np.array_equal(res.n_exceed, (res.null_errors >= res.reconstruction_errors).sum(axis=0))
    n_exceed, mean, p = gof_ref.reduce_null(res.reconstruction_errors, res.null_errors)
    assert np.array_equal(res.n_exceed, n_exceed) and np.array_equal(res.null_mean, mean) and np.array_equal(res.p_value, p)
    assert np.array_equal(res.p_value, (1 + res.n_exceed) / 6)
    for key in ("draw_s", "refit_s", "reduce_s", "total_s", "refit_kernel_ms"):
        assert res.timings[key] >= 0.0


def test_chunks_give_the_same_bits():
    X, W, alpha, whole = fitted(3)
    assert whole.timings["n_chunks"] == 1
    for per_chunk, n_chunks in ((1, 5), (2, 3)):
        res = sal.nb_goodness_of_fit(X, W, alpha, n_draws=5, seed=9, keep_draws=True, chunk_bytes=per_chunk * N * 96 * 8, **FIT)
        assert res.timings["n_chunks"] == n_chunks
        for name in ALL_NAMES:
            assert np.array_equal(getattr(res, name), getattr(whole, name)), (per_chunk, name)
    assert sal.nb_goodness_of_fit(X, W, alpha, n_draws=2, **FIT).draws is None


def test_planted_signature_and_calibration():
    """The 64 + 8 gamma-Poisson samples of tests/test_nbdraw_host.py at the defaults' convergence rule, with the host's bounds:
    mean p in [0.32, 0.68] (0.5 +- 5 x 0.289 / 8) and every planted sample at n_exceed = 0.  The device gives mean 0.488 and 2 of 64."""
    X, S, alpha = ref.calibration_samples()
    res = sal.nb_goodness_of_fit(X, S, alpha, n_draws=39, seed=0)
    null = res.p_value[:64]
    print(f"null samples: mean p {null.mean():.3f}, {int((null <= 0.05).sum())} of 64 at or below 0.05; planted n_exceed {res.n_exceed[64:]}; "
          f"iterations {res.n_iterations.min()}..{res.n_iterations.max()}, null {res.null_n_iterations.min()}..{res.null_n_iterations.max()}; "
          f"draw {res.timings['draw_s'] * 1e3:.2f} ms, refit {res.timings['refit_s'] * 1e3:.2f} ms")
    assert np.array_equal(res.n_exceed[64:], np.zeros(8, dtype=np.int32))
    assert 0.32 <= null.mean() <= 0.68


def test_errors_through_the_c_abi():
    lib = _lib.load_with_device()
    p = _lib.pointer
    X = np.ones((4, 10))
    H, err, nit, conv = np.empty((4, 97)), np.empty(4), np.empty(4, dtype=np.int32), np.empty(4, dtype=np.int32)
    exceed, mean, err_b, nit_b = np.empty(4, dtype=np.int32), np.empty(4), np.empty((5, 4)), np.empty((5, 4), dtype=np.int32)
    failed = np.zeros(1, dtype=np.int32)

    def gof(W, n_draws, alpha=20.0):
        return lib.salnmf_nb_goodness_of_fit(0, p(X), 4, 10, p(W), W.shape[0], p(np.full(4, alpha)), n_draws, 0, 10, 20, 10, 1e-7, 0, p(H), p(err), p(nit),
                                             p(conv), p(exceed), p(mean), p(err_b), p(nit_b), None, None, p(failed))

    assert gof(np.full((97, 10), 0.1), 5) == 1 and "n_signatures must be in [1, 96], got 97" in _lib.last_error()
    assert gof(np.full((3, 10), 0.1), 0) == 1 and "n_draws must be in [1, 65536], got 0" in _lib.last_error()
    assert gof(np.full((3, 10), 0.1), 5, alpha=0.0) == 1 and "dispersion must be finite and in (0, 1e+06]: sample 0 holds 0" in _lib.last_error()
    out = np.empty((5, 4, 10))

    def draw(W, n_draws, alpha=20.0):
        K = W.shape[0]
        return lib.salnmf_draw_nb_counts(0, p(np.ones((4, K))), 4, K, p(W), 10, p(np.full(4, alpha)), n_draws, 0, p(out), p(failed))

    assert draw(np.full((97, 10), 0.1), 5) == 1 and "n_signatures must be in [1, 96], got 97" in _lib.last_error()
    assert draw(np.full((3, 10), 0.1), 0) == 1 and "n_draws must be in [1, 65536], got 0" in _lib.last_error()
    assert draw(np.full((3, 10), 0.1), 5, alpha=0.0) == 1 and "dispersion must be finite and in (0, 1e+06]" in _lib.last_error()
    assert gof(np.full((3, 10), 0.1), 5) == 0 and draw(np.full((3, 10), 0.1), 5) == 0 and failed[0] == 0


def test_dispersion_test_on_overdispersed_and_on_poisson_data():
    """N = 16, K = 3, a 5-value grid, B = 19, data seed 0: the host replica (tests/_nbdraw_ref.py: dispersion_test, 300 steps) gives
    p = 1 / 20 and all 19 re-estimates at 10 on the alpha = 20 data, and the top of the grid with p = 0.65 on the Poisson data, so
    the first seed tried stands."""
    c = ref.DISPERSION_TEST
    X, W = ref.dispersion_test_data()
    res = sal.dispersion_test(X, W, grid=c["grid"], n_draws=c["B"], seed=0)
    print(f"alpha = 20 data: estimate {res.dispersion}, lr {res.lr_statistic:.1f}, p {res.p_value}, interval {res.dispersion_interval}, "
          f"bias {res.dispersion_bias}")
    assert res.p_value == 1 / 20 and not res.at_upper_edge
    assert res.dispersion_draws.shape == (19,) and res.dispersion_interval.shape == (3,)
    lo, hi = res.dispersion_interval[0], res.dispersion_interval[-1]
    assert lo <= 10.0 <= hi or lo <= 100.0 <= hi  # a grid neighbour of 20
    assert res.dispersion_bias == np.median(res.dispersion_draws) / res.dispersion
    X, W = ref.dispersion_test_data(poisson=True)
    res = sal.dispersion_test(X, W, grid=c["grid"], n_draws=c["B"], seed=0, interval=False)
    print(f"Poisson data: estimate {res.dispersion}, lr {res.lr_statistic:.3f}, p {res.p_value}")
    assert res.at_upper_edge and res.p_value > 0.05 and res.dispersion_draws is None
