"""``sal.nb_signature_presence_test`` on the device (``csrc/salnmf_nb_presence.h``): every solve bit for bit
``sal.nb_assign_signatures(candidates=A, required=A)``, every draw the replica's gamma-Poisson draw under the pair's counter words,
the reduction recomputed on the host, what a pair's results do not depend on, the calibration samples of
tests/test_nb_presence_host.py, and what the C entry point refuses."""

import numpy as np
import pytest

import _assign_masks_ref as masks_ref
import _nb_presence_ref as ref
import _nb_ref as nb_ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import _lib
from salamander_amd.nb import nb_constant

pytestmark = pytest.mark.gpu

N = 40  # two full tiles of 16 problems and a partial one per tested signature
B = 3
SEED = 12345678901234567
FIT = masks_ref.FIXED  # every solve is 20 steps long
CASES = [(1, 7), (3, 7), (17, 96), (96, 96)]
FIELDS = ("statistic", "p_value", "n_exceed", "tested", "exposures", "reconstruction_errors", "null_exposures", "null_errors", "null_statistics",
          "null_mean", "n_iterations", "converged", "null_n_iterations", "draws", "dispersion", "log_likelihood", "null_log_likelihood")
OBSERVED = ("statistic", "tested", "exposures", "reconstruction_errors", "null_exposures", "null_errors", "n_iterations", "converged", "log_likelihood",
            "null_log_likelihood")


def case(K, V):
    """(counts, signatures, dispersions, test, candidates): ``_nb_ref.catalogue`` rows (three zero-heavy ones) with totals 2, 1, 0, 257
    and 100 000 in rows 0..4, under ``_nb_ref.mixed_alpha`` (0.5, 20, 1e4 and 1e6 inside every tile); a signature row with zeros (the
    last, a tested one; row 3 is drawn from it); an (N, K) mask in which rows 5..8 do not hold test[0], row 9 holds test[1] alone and
    row 10 holds neither.  For K > 2 every other set holds signature 1, which is half uniform: without it a 20-step fit on a set that
    cannot reach a feature with counts grows past the draw's bound of 2^24, which test_errors_through_the_c_abi covers instead."""
    rng = np.random.default_rng(1000 * K + V)
    X, W = nb_ref.catalogue(N, K, V, seed=70 + K)
    W[K - 1, rng.permutation(V)[: max(2, V // 3)]] = 0.0
    if K > 1:  # signature 1 is dense in earnest: a null fit on {1} alone then stays a model that can be drawn from (mean total <= 2^24)
        W[1] = 0.5 * W[1] + 0.5 / V
    W = refit_ref.normalize(W)
    for row, total in ((0, 2), (1, 1), (2, 0), (3, 257), (4, 100000)):
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
    return X, W, nb_ref.mixed_alpha(N), test, C


_results = {}


def run_of(K, V):
    """One call per case, shared by the tests that read it (none changes it)."""
    if (K, V) not in _results:
        X, W, alpha, test, C = case(K, V)
        res = sal.nb_signature_presence_test(X, W, alpha, test, n_draws=B, seed=SEED, candidates=C, keep_draws=True, **FIT)
        _results[K, V] = (X, W, alpha, test, C, res)
    return _results[K, V]


def solve(X, W, alpha, A):
    """The contract's solve on the sets A, by the product's own assignment call."""
    return sal.nb_assign_signatures(X, W, alpha, candidates=A, required=A, **FIT)


def without(C, s):
    C0 = C.copy()
    C0[:, s] = False
    return C0


def same(a, b, names=FIELDS):
    for name in names:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name


@pytest.mark.parametrize("K,V", CASES)
def test_untested_pairs_and_shapes(K, V):
    X, W, alpha, test, C, res = run_of(K, V)
    S = len(test)
    want = ref.tested_pairs(C, test)
    assert isinstance(res, sal.NBPresenceResult) and np.array_equal(res.dispersion, alpha)
    assert res.tested.dtype == bool and np.array_equal(res.tested, want) and res.test == tuple(test) and np.array_equal(res.candidates, C)
    if K == 1:
        assert not want.any()
    else:
        assert not want[5:9, 0].any() and want[5:9, 1].all() and not want[9].any() and not want[10].any() and want[:5].all()
    for name in ("statistic", "p_value", "null_errors", "null_mean", "null_log_likelihood"):
        assert getattr(res, name).shape == (N, S) and np.array_equal(np.isnan(getattr(res, name)), ~want), name
    assert res.null_statistics.shape == (B, N, S) and np.array_equal(np.isnan(res.null_statistics), np.broadcast_to(~want, (B, N, S)))
    assert res.null_exposures.shape == (N, S, K) and np.array_equal(np.isnan(res.null_exposures).all(axis=2), ~want)
    assert res.draws.shape == (B, N, S, V) and not res.draws[:, ~want].any()
    assert not res.n_exceed[~want].any() and not res.n_iterations[~want].any() and not res.null_n_iterations[:, ~want].any()
    none = ~want.any(axis=1)
    assert np.array_equal(np.isnan(res.exposures).all(axis=1), none) and np.array_equal(np.isnan(res.reconstruction_errors), none)
    assert np.array_equal(np.isnan(res.log_likelihood), none)
    assert res.n_iterations.dtype == np.int32 and res.n_exceed.dtype == np.int32 and res.converged.dtype == bool


@pytest.mark.parametrize("K,V", CASES[1:])
def test_observed_fits_are_the_two_masked_solves(K, V):
    X, W, alpha, test, C, res = run_of(K, V)
    rows = np.flatnonzero(res.tested.any(axis=1))
    alt = solve(X[rows], W, alpha[rows], C[rows])
    assert np.array_equal(res.exposures[rows], alt.exposures) and np.array_equal(res.reconstruction_errors[rows], alt.reconstruction_errors)
    assert (res.exposures[rows][~C[rows]] == 0.0).all()
    for j, s in enumerate(test):
        rows = np.flatnonzero(res.tested[:, j])
        alt, null = solve(X[rows], W, alpha[rows], C[rows]), solve(X[rows], W, alpha[rows], without(C[rows], s))
        assert np.array_equal(res.null_exposures[rows, j], null.exposures), s
        assert np.array_equal(res.null_errors[rows, j], null.reconstruction_errors), s
        assert np.array_equal(res.statistic[rows, j], null.reconstruction_errors - alt.reconstruction_errors), s
        assert np.array_equal(res.n_iterations[rows, j], np.stack([alt.n_iterations, null.n_iterations], axis=1)), s
        assert np.array_equal(res.converged[rows, j], np.stack([alt.converged, null.converged], axis=1)), s
        assert (res.null_exposures[rows, j, s] == 0.0).all()
    const = nb_constant(X, alpha)
    assert np.array_equal(res.log_likelihood, -res.reconstruction_errors + const, equal_nan=True)
    assert np.array_equal(res.null_log_likelihood, -res.null_errors + const[:, None], equal_nan=True)


@pytest.mark.parametrize("K,V", CASES[2:])
def test_without_candidates_the_alternative_is_the_refit(K, V):
    X, W, alpha, test, _ = case(K, V)
    res = sal.nb_signature_presence_test(X, W, alpha, test, n_draws=1, seed=SEED, **FIT)
    fit = sal.nb_refit_exposures(X, W, alpha, **FIT)
    assert res.candidates is None and res.tested.all() and res.draws is None
    assert np.array_equal(res.exposures, fit.exposures) and np.array_equal(res.reconstruction_errors, fit.reconstruction_errors)
    assert np.array_equal(res.n_iterations[:, 0, 0], fit.n_iterations) and np.array_equal(res.converged[:, 0, 0], fit.converged)
    assert np.array_equal(res.log_likelihood, fit.log_likelihood)


@pytest.mark.parametrize("K,V", CASES[1:])
def test_draws_equal_the_replica(K, V):
    X, W, alpha, test, C, res = run_of(K, V)
    want = ref.draws_from(res.null_exposures, refit_ref.normalize(W), alpha, test, res.tested, B, SEED)
    assert np.array_equal(res.draws, want)
    totals = res.draws.sum(axis=3)
    assert (totals[:, res.tested] != np.broadcast_to(X.sum(axis=1)[:, None], res.tested.shape)[res.tested]).any()  # unconditional: the totals vary
    assert not np.array_equal(res.draws[0, 4, 0], res.draws[0, 4, 1]) and not np.array_equal(res.draws[0, 4, 0], res.draws[1, 4, 0])


@pytest.mark.parametrize("K,V", CASES[1:])
def test_null_statistics_are_the_two_solves_of_the_kept_draws(K, V):
    X, W, alpha, test, C, res = run_of(K, V)
    for j, s in enumerate(test):
        rows = np.flatnonzero(res.tested[:, j])
        for b in range(B):
            drawn = res.draws[b, rows, j]
            alt, null = solve(drawn, W, alpha[rows], C[rows]), solve(drawn, W, alpha[rows], without(C[rows], s))
            assert np.array_equal(res.null_statistics[b, rows, j], null.reconstruction_errors - alt.reconstruction_errors), (s, b)
            assert np.array_equal(res.null_n_iterations[b, rows, j], np.stack([alt.n_iterations, null.n_iterations], axis=1)), (s, b)


@pytest.mark.parametrize("K,V", CASES[1:])
def test_reduction(K, V):
    res = run_of(K, V)[5]
    n_exceed, mean, p = ref.reduce_null(res.statistic, res.null_statistics)
    assert np.array_equal(res.n_exceed, n_exceed) and np.array_equal(res.null_mean, mean, equal_nan=True) and np.array_equal(res.p_value, p, equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res.n_exceed, (res.null_statistics >= res.statistic).sum(axis=0))
    assert np.array_equal(res.p_value[res.tested], (1 + res.n_exceed[res.tested]) / (B + 1))
    for key in ("draw_s", "solve_s", "reduce_s", "total_s", "presence_kernel_ms"):
        assert res.timings[key] >= 0.0
    assert res.timings["n_chunks"] == 1


@pytest.mark.parametrize("K,V", CASES[1:])
def test_a_pair_does_not_depend_on_what_else_is_tested_or_on_the_number_of_draws(K, V):
    X, W, alpha, test, C = case(K, V)
    both = sal.nb_signature_presence_test(X, W, alpha, test, n_draws=8, seed=3, candidates=C, keep_draws=True, **FIT)
    one = sal.nb_signature_presence_test(X, W, alpha, [K - 1], n_draws=4, seed=3, candidates=C, keep_draws=True, **FIT)
    for name in ("statistic", "tested", "null_errors", "null_exposures", "n_iterations", "converged", "null_log_likelihood"):
        assert np.array_equal(getattr(one, name)[:, 0], getattr(both, name)[:, 1], equal_nan=True), name
    rows = one.tested[:, 0]  # (a sample whose only tested pair is the other signature's has no alternative fit here)
    assert np.array_equal(one.exposures[rows], both.exposures[rows]) and np.array_equal(one.reconstruction_errors[rows], both.reconstruction_errors[rows])
    for name in ("null_statistics", "null_n_iterations", "draws"):
        assert np.array_equal(getattr(one, name)[:, :, 0], getattr(both, name)[:4, :, 1], equal_nan=True), name  # B = 4 against B = 8, S = 1 against S = 2
    assert not np.array_equal(both.draws[:, :5, 0], both.draws[:, :5, 1])


def test_chunks_give_the_same_bits():
    X, W, alpha, test, C, whole = run_of(3, 7)
    pairs = int(whole.tested.sum())
    for per_chunk, n_chunks in ((1, 3), (2, 2), (3, 1)):
        res = sal.nb_signature_presence_test(X, W, alpha, test, n_draws=B, seed=SEED, candidates=C, keep_draws=True,
                                             chunk_bytes=per_chunk * pairs * 7 * 8, **FIT)
        assert res.timings["n_chunks"] == n_chunks
        same(res, whole)
    assert sal.nb_signature_presence_test(X, W, alpha, test, n_draws=2, **FIT).draws is None


def test_row_permutations_single_rows_and_scalar_dispersion():
    X, W, alpha, test, C, whole = run_of(17, 96)
    perm = np.random.default_rng(5).permutation(N)
    res = sal.nb_signature_presence_test(X[perm], W, alpha[perm], test, n_draws=1, seed=SEED, candidates=C[perm], **FIT)
    for name in OBSERVED:  # (the draws carry the row's index in their counter: another row, another draw)
        assert np.array_equal(getattr(res, name), getattr(whole, name)[perm], equal_nan=True), name
    for n in (0, 4, 7, 39):
        one = sal.nb_signature_presence_test(X[n:n + 1], W, alpha[n], test, n_draws=B, seed=SEED, candidates=C[n:n + 1], keep_draws=True, **FIT)
        for name in OBSERVED:
            assert np.array_equal(getattr(one, name)[0], getattr(whole, name)[n], equal_nan=True), (n, name)
        if n == 0:  # the same row word: the same draws
            for name in ("draws", "null_statistics", "null_n_iterations"):
                assert np.array_equal(getattr(one, name)[:, 0], getattr(whole, name)[:, 0], equal_nan=True), name
            assert np.array_equal(one.n_exceed[0], whole.n_exceed[0]) and np.array_equal(one.null_mean[0], whole.null_mean[0])
    scalar = sal.nb_signature_presence_test(X, W, 20.0, test, n_draws=B, seed=SEED, candidates=C, keep_draws=True, **FIT)
    array = sal.nb_signature_presence_test(X, W, np.full(N, 20.0), test, n_draws=B, seed=SEED, candidates=C, keep_draws=True, **FIT)
    same(scalar, array)
    assert not np.array_equal(scalar.statistic, whole.statistic, equal_nan=True)


def test_planted_signature_and_calibration():
    """The 64 + 8 gamma-Poisson samples of tests/test_nb_presence_host.py at the defaults' convergence rule, under the same two caps
    (the device's solves stop on their own tests, the replica's at a fixed step count: bounds, not equalities).  The device gives 3 of
    64 at or below 0.05, all 8 planted samples at n_exceed 0, their statistics 113 to 277 times the largest null one."""
    X, S, s, alpha = ref.calibration_samples()
    res = sal.nb_signature_presence_test(X, S, alpha, [s], n_draws=ref.CALIBRATION_DRAWS, seed=0)
    null = res.p_value[:64, 0]
    ratio = res.statistic[64:, 0] / res.null_statistics[:, 64:, 0].max(axis=0)
    print(f"null samples: {int((null <= 0.05).sum())} of 64 at or below 0.05, mean p {null.mean():.3f}; planted n_exceed {res.n_exceed[64:, 0]}, "
          f"statistic / largest null {ratio.min():.1f} .. {ratio.max():.1f}; iterations {res.n_iterations.min()}..{res.n_iterations.max()}, "
          f"null {res.null_n_iterations.min()}..{res.null_n_iterations.max()}; solve {res.timings['solve_s']:.3f} s")
    assert res.tested.all()
    assert (null <= 0.05).sum() <= ref.CALIBRATION_CAP
    assert np.array_equal(res.n_exceed[64:, 0], np.zeros(8, dtype=np.int32))


def test_errors_through_the_c_abi():
    lib = _lib.load_with_device()
    p = _lib.pointer
    out = dict(tested=np.empty((4, 2), dtype=np.uint8), stat=np.empty((4, 2)), exceed=np.empty((4, 2), dtype=np.int32), mean=np.empty((4, 2)),
               H=np.empty((4, 97)), err=np.empty(4), H0=np.empty((4, 2, 97)), err0=np.empty((4, 2)), nit=np.empty((4, 2, 2), dtype=np.int32),
               conv=np.empty((4, 2, 2), dtype=np.int32), stat_b=np.empty((5, 4, 2)), nit_b=np.empty((5, 4, 2, 2), dtype=np.int32))
    failed = np.full(1, -1, dtype=np.int32)

    def call(W, test, n_draws, max_it=20, alpha=20.0, X=np.ones((4, 10))):
        t = np.array(test, dtype=np.int32)
        a = np.full(4, alpha)
        return lib.salnmf_nb_signature_presence(0, p(X), 4, 10, p(W), W.shape[0], p(a), p(t), t.size, None, n_draws, 0, 10, max_it, 10, 1e-7, 0,
                                                *(p(o) for o in out.values()), None, None, p(failed))

    W = np.full((3, 10), 0.1)
    assert call(np.full((97, 10), 0.1), [0, 1], 5) == 1 and "n_signatures must be in [1, 96], got 97" in _lib.last_error()
    assert call(W, [0, 1], 0) == 1 and "n_draws must be in [1, 65536], got 0" in _lib.last_error()
    assert call(W, [0, 3], 5) == 1 and "tested signature 3 is not in [0, 3)" in _lib.last_error()
    assert call(W, [1, 1], 5) == 1 and "signature 1 is tested twice" in _lib.last_error()
    assert call(W, [0, 1], 5, max_it=25) == 1 and "max_iterations must be a multiple of conv_test_freq, got 25 and 10" in _lib.last_error()
    assert call(W, [0, 1], 5, alpha=0.0) == 1 and "dispersion must be finite and in (0, 1e+06]: sample 0 holds 0" in _lib.last_error()
    assert call(W, [0, 1], 5, alpha=2e6) == 1 and "dispersion must be finite and in (0, 1e+06]: sample 0 holds 2e+06" in _lib.last_error()
    big = np.ones((4, 10))
    big[2, 0] = 2.0**25
    assert call(W, [0, 1], 5, X=big) == 1 and "the null fits' row sums must not exceed 2^24: sample 2 without signature 0" in _lib.last_error()
    assert call(W, [0, 1], 5) == 0 and failed[0] == 0 and out["tested"].all() and np.isfinite(out["stat"]).all() and np.isfinite(out["stat_b"]).all()
