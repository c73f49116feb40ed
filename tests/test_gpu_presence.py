"""``sal.signature_presence_test`` on the device: the observed and the null fits against the two
``sal.assign_signatures(candidates=A, required=A)`` calls of the contract, the draws against the host replica
(tests/_presence_ref.py) from the device's own null exposures, the reduction against its stated rules -- every comparison
``np.array_equal`` -- and the calibration samples of tests/test_presence_host.py."""

import numpy as np
import pytest

import _presence_ref as ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import _lib

pytestmark = pytest.mark.gpu

N = 40  # two full tiles of 16 problems and a partial one per tested signature
B = 3
SEED = 12345678901234567
FIT = dict(min_iterations=20, max_iterations=60, conv_test_freq=10, tol=1e-5)
CASES = [(1, 7), (3, 7), (17, 96), (96, 96)]


def case(K, V):
    """(counts, signatures, test, candidates): Poisson counts with three zero-heavy rows and totals 0, 1, 2, 257 and 100 000; a
    signature row with zeros (the last, a tested one; row 3 is drawn from it); an (N, K) mask in which rows 5..8 do not hold
    test[0], row 9 holds test[1] alone and row 10 holds neither.  For K > 2 every other set holds the dense signature 1, so no
    feature with counts is left without a signature."""
    rng = np.random.default_rng(1000 * K + V)
    X, W = refit_ref.poisson_catalogue(N, K, V=V, seed=70 + K, zero_heavy=3)
    W[K - 1, rng.permutation(V)[: max(2, V // 3)]] = 0.0
    W = refit_ref.normalize(W)
    X[0] = 0.0
    for row, total in ((1, 1), (2, 2), (3, 257), (4, 100000)):
        X[row] = rng.multinomial(total, W[K - 1] if row == 3 else np.full(V, 1.0 / V))
    test = [0] if K == 1 else [0, K - 1]
    C = rng.random((N, K)) < 0.8
    C[:, test] = True
    C[:, min(1, K - 1)] = True
    C[:5] = True
    C[5:9, test[0]] = K == 1
    C[9] = False
    C[9, test[-1]] = True
    if K > 2:
        C[10] = False
        C[10, 1] = True
    return X, W, test, C


_results = {}


def run_of(K, V):
    """One call per case, shared by the tests that read it (none changes it)."""
    if (K, V) not in _results:
        X, W, test, C = case(K, V)
        _results[K, V] = (X, W, test, C, sal.signature_presence_test(X, W, test, n_draws=B, seed=SEED, candidates=C, keep_draws=True, **FIT))
    return _results[K, V]


def solve(X, W, A):
    """The contract's solve on the sets A, by the product's own assignment call."""
    return sal.assign_signatures(X, W, candidates=A, required=A, **FIT)


def without(C, s):
    C0 = C.copy()
    C0[:, s] = False
    return C0


@pytest.mark.parametrize("K,V", CASES)
def test_untested_pairs_and_shapes(K, V):
    X, W, test, C, res = run_of(K, V)
    S = len(test)
    want = ref.tested_pairs(C, test)
    assert res.tested.dtype == bool and np.array_equal(res.tested, want) and res.test == tuple(test) and np.array_equal(res.candidates, C)
    if K == 1:
        assert not want.any()
    else:
        assert not want[5:9, 0].any() and want[5:9, 1].all() and not want[9].any() and not want[10].any() and want[:5].all()
    for name in ("statistic", "p_value", "null_errors", "null_mean"):
        assert getattr(res, name).shape == (N, S) and np.array_equal(np.isnan(getattr(res, name)), ~want), name
    assert res.null_statistics.shape == (B, N, S) and np.array_equal(np.isnan(res.null_statistics), np.broadcast_to(~want, (B, N, S)))
    assert res.null_exposures.shape == (N, S, K) and np.array_equal(np.isnan(res.null_exposures).all(axis=2), ~want)
    assert res.draws.shape == (B, N, S, V) and not res.draws[:, ~want].any()
    assert not res.n_exceed[~want].any() and not res.n_iterations[~want].any() and not res.null_n_iterations[:, ~want].any()
    assert np.array_equal(np.isnan(res.exposures).all(axis=1), ~want.any(axis=1)) and np.array_equal(np.isnan(res.reconstruction_errors), ~want.any(axis=1))
    assert res.n_iterations.dtype == np.int32 and res.n_exceed.dtype == np.int32 and res.converged.dtype == bool


@pytest.mark.parametrize("K,V", CASES[1:])
def test_observed_fits_are_the_two_masked_solves(K, V):
    X, W, test, C, res = run_of(K, V)
    rows = np.flatnonzero(res.tested.any(axis=1))
    alt = solve(X[rows], W, C[rows])
    assert np.array_equal(res.exposures[rows], alt.exposures) and np.array_equal(res.reconstruction_errors[rows], alt.reconstruction_errors)
    assert (res.exposures[rows][~C[rows]] == 0.0).all()
    for j, s in enumerate(test):
        rows = np.flatnonzero(res.tested[:, j])
        alt, null = solve(X[rows], W, C[rows]), solve(X[rows], W, without(C[rows], s))
        assert np.array_equal(res.null_exposures[rows, j], null.exposures), s
        assert np.array_equal(res.null_errors[rows, j], null.reconstruction_errors), s
        assert np.array_equal(res.statistic[rows, j], null.reconstruction_errors - alt.reconstruction_errors), s
        assert np.array_equal(res.n_iterations[rows, j], np.stack([alt.n_iterations, null.n_iterations], axis=1)), s
        assert np.array_equal(res.converged[rows, j], np.stack([alt.converged, null.converged], axis=1)), s
        assert (res.null_exposures[rows, j, s] == 0.0).all()
    assert 1 < np.unique(res.n_iterations[res.tested]).size  # problems of one tile stop at different tests
    assert not res.converged[res.tested].all() and res.converged[res.tested].any()


@pytest.mark.parametrize("K,V", CASES[1:])
def test_draws_equal_the_replica(K, V):
    X, W, test, C, res = run_of(K, V)
    want = ref.draws_from(res.null_exposures, refit_ref.normalize(W), X.sum(axis=1), test, res.tested, B, SEED)
    assert np.array_equal(res.draws, want)
    assert np.array_equal(res.draws.sum(axis=3), np.where(res.tested, X.sum(axis=1)[:, None], 0.0)[None].repeat(B, axis=0))
    assert not np.array_equal(res.draws[0, 4, 0], res.draws[0, 4, 1]) and not np.array_equal(res.draws[0, 4, 0], res.draws[1, 4, 0])


@pytest.mark.parametrize("K,V", CASES[1:])
def test_null_statistics_are_the_two_solves_of_the_kept_draws(K, V):
    X, W, test, C, res = run_of(K, V)
    for j, s in enumerate(test):
        rows = np.flatnonzero(res.tested[:, j])
        for b in range(B):
            drawn = res.draws[b, rows, j]
            alt, null = solve(drawn, W, C[rows]), solve(drawn, W, without(C[rows], s))
            assert np.array_equal(res.null_statistics[b, rows, j], null.reconstruction_errors - alt.reconstruction_errors), (s, b)
            assert np.array_equal(res.null_n_iterations[b, rows, j], np.stack([alt.n_iterations, null.n_iterations], axis=1)), (s, b)


@pytest.mark.parametrize("K,V", CASES[1:])
def test_reduction(K, V):
    _, _, _, _, res = run_of(K, V)
    n_exceed, mean, p = ref.reduce_null(res.statistic, res.null_statistics)
    assert np.array_equal(res.n_exceed, n_exceed) and np.array_equal(res.null_mean, mean, equal_nan=True) and np.array_equal(res.p_value, p, equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res.n_exceed, (res.null_statistics >= res.statistic).sum(axis=0))
    assert np.array_equal(res.p_value[res.tested], (1 + res.n_exceed[res.tested]) / (B + 1))
    assert 1 < np.unique(res.n_exceed[res.tested]).size
    for key in ("draw_s", "solve_s", "reduce_s", "total_s", "presence_kernel_ms"):
        assert res.timings[key] >= 0.0
    assert res.timings["n_chunks"] == 1


def test_a_pair_does_not_depend_on_what_else_is_tested_or_on_the_number_of_draws():
    X, W, _, _ = case(17, 96)
    both = sal.signature_presence_test(X, W, [0, 2], n_draws=8, seed=3, keep_draws=True, **FIT)
    one = sal.signature_presence_test(X, W, [2], n_draws=4, seed=3, keep_draws=True, **FIT)
    assert both.candidates is None and both.tested.all()
    for name in ("statistic", "null_errors", "null_exposures", "n_iterations", "converged"):
        assert np.array_equal(getattr(one, name)[:, 0], getattr(both, name)[:, 1]), name
    assert np.array_equal(one.exposures, both.exposures) and np.array_equal(one.reconstruction_errors, both.reconstruction_errors)
    assert np.array_equal(one.exposures, sal.assign_signatures(X, W, candidates=np.ones(17, dtype=bool), required=np.ones(17, dtype=bool), **FIT).exposures)
    for name in ("null_statistics", "null_n_iterations", "draws"):
        assert np.array_equal(getattr(one, name)[:, :, 0], getattr(both, name)[:4, :, 1]), name  # B = 4 against B = 8, S = 1 against S = 2
    assert not np.array_equal(both.draws[:, :, 0], both.draws[:, :, 1])
    assert not np.array_equal(sal.signature_presence_test(X, W, [2], n_draws=1, seed=4, keep_draws=True, **FIT).draws[0], one.draws[0])


def test_chunks_give_the_same_bits():
    X, W, test, C, whole = run_of(3, 7)
    pairs = int(whole.tested.sum())
    for per_chunk, n_chunks in ((1, 3), (2, 2)):
        res = sal.signature_presence_test(X, W, test, n_draws=B, seed=SEED, candidates=C, keep_draws=True, chunk_bytes=per_chunk * pairs * 7 * 8, **FIT)
        assert res.timings["n_chunks"] == n_chunks
        for name in ("statistic", "p_value", "n_exceed", "tested", "exposures", "reconstruction_errors", "null_exposures", "null_errors",
                     "null_statistics", "null_mean", "n_iterations", "converged", "null_n_iterations", "draws"):
            assert np.array_equal(getattr(res, name), getattr(whole, name), equal_nan=True), (per_chunk, name)
    assert sal.signature_presence_test(X, W, test, n_draws=2, **FIT).draws is None


def test_planted_signature_and_calibration():
    """The 64 + 8 samples of tests/test_presence_host.py at the defaults' convergence rule, under the same two conditions (the
    device's solves stop on their own tests, the replica's at a fixed step count: bounds, not equalities).  The device gives 6 of
    64 at or below 0.05, all 8 planted samples at n_exceed 0, their statistics 146 to 385 times the largest null one."""
    X, S, s = ref.calibration_samples()
    res = sal.signature_presence_test(X, S, [s], n_draws=39, seed=0)
    null = res.p_value[:64, 0]
    ratio = res.statistic[64:, 0] / res.null_statistics[:, 64:, 0].max(axis=0)
    print(f"null samples: {int((null <= 0.05).sum())} of 64 at or below 0.05, mean p {null.mean():.3f}; planted n_exceed {res.n_exceed[64:, 0]}, "
          f"statistic / largest null {ratio.min():.1f} .. {ratio.max():.1f}; iterations {res.n_iterations.min()}..{res.n_iterations.max()}, "
          f"null {res.null_n_iterations.min()}..{res.null_n_iterations.max()}; smallest statistic {res.statistic.min():.3g}")
    assert res.tested.all()
    assert (null <= 0.05).sum() <= 8
    assert np.array_equal(res.n_exceed[64:, 0], np.zeros(8, dtype=np.int32))
    assert np.array_equal(res.p_value[64:, 0], np.full(8, 1 / 40))


def test_errors_through_the_c_abi():
    lib = _lib.load_with_device()
    p = _lib.pointer
    X = np.ones((4, 10))
    out = dict(tested=np.empty((4, 2), dtype=np.uint8), stat=np.empty((4, 2)), exceed=np.empty((4, 2), dtype=np.int32), mean=np.empty((4, 2)),
               H=np.empty((4, 97)), err=np.empty(4), H0=np.empty((4, 2, 97)), err0=np.empty((4, 2)), nit=np.empty((4, 2, 2), dtype=np.int32),
               conv=np.empty((4, 2, 2), dtype=np.int32), stat_b=np.empty((5, 4, 2)), nit_b=np.empty((5, 4, 2, 2), dtype=np.int32))

    def call(W, test, n_draws, max_it=20):
        t = np.array(test, dtype=np.int32)
        return lib.salnmf_signature_presence(0, p(X), 4, 10, p(W), W.shape[0], p(t), t.size, None, n_draws, 0, 10, max_it, 10, 1e-7, 0,
                                             *(p(a) for a in out.values()), None, None)

    W = np.full((3, 10), 0.1)
    assert call(np.full((97, 10), 0.1), [0, 1], 5) == 1 and "n_signatures must be in [1, 96], got 97" in _lib.last_error()
    assert call(W, [0, 1], 0) == 1 and "n_draws must be in [1, 65536], got 0" in _lib.last_error()
    assert call(W, [0, 3], 5) == 1 and "tested signature 3 is not in [0, 3)" in _lib.last_error()
    assert call(W, [1, 1], 5) == 1 and "signature 1 is tested twice" in _lib.last_error()
    assert call(W, [0, 1], 5, max_it=25) == 1 and "max_iterations must be a multiple of conv_test_freq, got 25 and 10" in _lib.last_error()
    assert call(W, [0, 1], 5) == 0 and out["tested"].all() and np.isfinite(out["stat"]).all() and np.isfinite(out["stat_b"]).all()
