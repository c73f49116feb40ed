"""``sal.draw_model_counts`` and ``sal.goodness_of_fit`` on the device: the draws against the host
replica (tests/_gof_ref.py), the observed and the null fits against ``sal.refit_exposures``, the reduction against its stated
rules -- every comparison ``np.array_equal`` -- and the calibration samples of tests/test_gof_host.py."""

import numpy as np
import pytest

import _gof_ref as ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import _lib

pytestmark = pytest.mark.gpu

EPS = refit_ref.EPSILON
N = 40  # two full tiles of 16 problems and a partial one
FIT = dict(min_iterations=20, max_iterations=60, conv_test_freq=10, tol=1e-5)
FIT_NAMES = ("exposures", "reconstruction_errors", "n_iterations", "converged")


def draw_case(K, V, seed):
    """Exposures with entries at exactly EPSILON and at 0 (one row all zero), a signature row with zeros, and totals at 0, 1, 2,
    the 256-lane boundary and 100 000."""
    rng = np.random.default_rng(seed)
    W = rng.dirichlet(np.full(V, 0.3), size=K)
    W[K // 2, rng.permutation(V)[: max(2, V // 3)]] = 0.0
    H = rng.uniform(0.01, 500.0, size=(N, K))
    H[rng.random((N, K)) < 0.15] = EPS
    H[rng.random((N, K)) < 0.05] = 0.0
    H[11] = 0.0
    totals = rng.integers(3, 3000, size=N).astype(np.float64)
    totals[:7] = (0, 1, 2, 255, 256, 257, 100000)
    return H, W, totals


@pytest.mark.parametrize("K,V", [(1, 7), (3, 7), (17, 96), (96, 96)])
def test_draws_equal_the_replica(K, V):
    H, W, totals = draw_case(K, V, seed=100 * K + V)
    got = sal.draw_model_counts(H, W, totals, 3, seed=12345678901234567)
    want = ref.draw_model_counts(H, W, totals, 3, seed=12345678901234567)
    assert got.shape == (3, N, V) and got.dtype == np.float64
    assert np.array_equal(got, want)
    live = np.flatnonzero(H.sum(axis=1) > 0)
    assert np.array_equal(got[:, live].sum(axis=2), np.broadcast_to(totals[live], (3, live.size)))
    assert not got[:, 11].any() and not got[:, 0].any()
    assert not got[:, :, (W == 0).all(axis=0)].any()  # cells of weight 0 stay 0 (K = 1: the zeros of the signature)


def test_draw_b_does_not_depend_on_the_number_of_draws():
    H, W, totals = draw_case(17, 96, seed=5)
    d8 = sal.draw_model_counts(H, W, totals, 8, seed=3)
    assert np.array_equal(sal.draw_model_counts(H, W, totals, 4, seed=3), d8[:4])
    assert not np.array_equal(d8[0], d8[1]) and not np.array_equal(sal.draw_model_counts(H, W, totals, 1, seed=4)[0], d8[0])


def count_case(K):
    """Poisson counts with three zero-heavy rows, one row with a single mutation and one all-zero row."""
    X, W = refit_ref.poisson_catalogue(N, K, V=96, seed=40 + K, zero_heavy=3)
    X[1] = 0.0
    X[1, 48] = 1.0
    X[2] = 0.0
    return X, W


_results = {}


def fitted(K):
    """One goodness_of_fit call per K, shared by the tests that read it (none changes it)."""
    if K not in _results:
        X, W = count_case(K)
        _results[K] = (X, W, sal.goodness_of_fit(X, W, n_draws=5, seed=9, keep_draws=True, **FIT))
    return _results[K]


@pytest.mark.parametrize("K", [3, 17])
def test_observed_fit_is_the_refit(K):
    X, W, res = fitted(K)
    want = sal.refit_exposures(X, W, **FIT)
    for name in FIT_NAMES:
        assert np.array_equal(getattr(res, name), getattr(want, name)), name
    assert res.n_iterations.dtype == np.int32 and res.converged.dtype == bool


@pytest.mark.parametrize("K", [3, 17])
def test_null_fits_are_refits_of_the_draws(K):
    X, W, res = fitted(K)
    assert res.draws.shape == (5, N, 96) and res.null_errors.shape == (5, N) and res.null_n_iterations.shape == (5, N)
    assert np.array_equal(res.draws, sal.draw_model_counts(res.exposures, W, X.sum(axis=1), 5, 9))
    assert np.array_equal(res.draws, ref.draw_model_counts(res.exposures, W, X.sum(axis=1), 5, 9))
    assert np.array_equal(res.draws.sum(axis=2), np.broadcast_to(X.sum(axis=1), (5, N)))
    for b in range(5):
        one = sal.refit_exposures(res.draws[b], W, **FIT)
        assert np.array_equal(res.null_errors[b], one.reconstruction_errors), b
        assert np.array_equal(res.null_n_iterations[b], one.n_iterations), b
    assert 1 < np.unique(res.null_n_iterations).size  # problems of one tile stop at different tests


@pytest.mark.parametrize("K", [3, 17])
def test_reduction(K):
    X, W, res = fitted(K)
    assert not res.converged.all()  # a row that ran into max_iterations is compared like every other
    assert res.n_exceed.dtype == np.int32
    assert np.array_equal(res.n_exceed, (res.null_errors >= res.reconstruction_errors).sum(axis=0))
    n_exceed, mean, p = ref.reduce_null(res.reconstruction_errors, res.null_errors)
    assert np.array_equal(res.n_exceed, n_exceed) and np.array_equal(res.null_mean, mean) and np.array_equal(res.p_value, p)
    assert np.array_equal(res.p_value, (1 + res.n_exceed) / 6)
    assert 1 < np.unique(res.n_exceed).size
    for key in ("draw_s", "refit_s", "reduce_s", "total_s", "refit_kernel_ms"):
        assert res.timings[key] >= 0.0


def test_chunks_give_the_same_bits():
    X, W, whole = fitted(3)
    assert whole.timings["n_chunks"] == 1
    for per_chunk, n_chunks in ((1, 5), (2, 3)):
        res = sal.goodness_of_fit(X, W, n_draws=5, seed=9, keep_draws=True, chunk_bytes=per_chunk * N * 96 * 8, **FIT)
        assert res.timings["n_chunks"] == n_chunks
        for name in FIT_NAMES + ("n_exceed", "p_value", "null_mean", "null_errors", "null_n_iterations", "draws"):
            assert np.array_equal(getattr(res, name), getattr(whole, name)), (per_chunk, name)
    assert sal.goodness_of_fit(X, W, n_draws=2, **FIT).draws is None


def test_planted_signature_and_calibration():
    """The 64 + 8 samples of tests/test_gof_host.py at the defaults' convergence rule: the same bounds as on the host (the
    device's refits stop on their own tests, the replica's at a fixed step count: bounds, not equalities).  The device gives mean
    0.582 and 3 of 64."""
    X, S = ref.calibration_samples()
    res = sal.goodness_of_fit(X, S, n_draws=39, seed=0)
    null = res.p_value[:64]
    print(f"null samples: mean p {null.mean():.3f}, {int((null <= 0.05).sum())} of 64 at or below 0.05; planted n_exceed {res.n_exceed[64:]}; "
          f"iterations {res.n_iterations.min()}..{res.n_iterations.max()}, null {res.null_n_iterations.min()}..{res.null_n_iterations.max()}")
    assert np.array_equal(res.n_exceed[64:], np.zeros(8, dtype=np.int32))
    assert np.array_equal(res.p_value[64:], np.full(8, 1 / 40))
    assert 0.3 <= null.mean() <= 0.7
    assert (null <= 0.05).sum() <= 8


def test_errors_through_the_c_abi():
    lib = _lib.load_with_device()
    p = _lib.pointer
    X = np.ones((4, 10))
    H, err, nit, conv = np.empty((4, 97)), np.empty(4), np.empty(4, dtype=np.int32), np.empty(4, dtype=np.int32)
    exceed, mean, err_b, nit_b = np.empty(4, dtype=np.int32), np.empty(4), np.empty((5, 4)), np.empty((5, 4), dtype=np.int32)

    def gof(W, n_draws):
        return lib.salnmf_goodness_of_fit(0, p(X), 4, 10, p(W), W.shape[0], n_draws, 0, 10, 20, 10, 1e-7, 0, p(H), p(err), p(nit), p(conv), p(exceed),
                                          p(mean), p(err_b), p(nit_b), None, None)

    assert gof(np.full((97, 10), 0.1), 5) == 1 and "n_signatures must be in [1, 96], got 97" in _lib.last_error()
    assert gof(np.full((3, 10), 0.1), 0) == 1 and "n_draws must be in [1, 65536], got 0" in _lib.last_error()
    out = np.empty((5, 4, 10))

    def draw(W, n_draws):
        K = W.shape[0]
        return lib.salnmf_draw_model_counts(0, p(np.ones((4, K))), 4, K, p(W), 10, p(np.full(4, 3.0)), n_draws, 0, p(out))

    assert draw(np.full((97, 10), 0.1), 5) == 1 and "n_signatures must be in [1, 96], got 97" in _lib.last_error()
    assert draw(np.full((3, 10), 0.1), 0) == 1 and "n_draws must be in [1, 65536], got 0" in _lib.last_error()
    assert gof(np.full((3, 10), 0.1), 5) == 0 and draw(np.full((3, 10), 0.1), 5) == 0 and np.array_equal(out.sum(axis=2), np.full((5, 4), 3.0))
