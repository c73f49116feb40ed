"""``sal.signature_power`` on the device: the presence part against ``sal.signature_presence_test``, the
planted exposures and the alternative draws against the host replica (tests/_power_ref.py) from the device's own arrays, the
alternative statistics against the two ``sal.assign_signatures(candidates=A, required=A)`` calls of the contract on the kept
draws, the reduction against its stated rules -- every comparison ``np.array_equal`` -- and the calibration samples of
tests/test_power_host.py."""

import numpy as np
import pytest

import _power_ref as ref
import _presence_ref as presence_ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import _lib

pytestmark = pytest.mark.gpu

N = 12
B = 3
A = 2
SHARES = (0.0, 0.25)
ALPHA = 0.5  # max_exceed = 1: (1 + 1) / 4 <= 0.5 < (1 + 2) / 4
SEED = 12345678901234567
FIT = dict(min_iterations=20, max_iterations=60, conv_test_freq=10, tol=1e-5)
CASES = [(1, 7), (3, 7), (17, 96), (96, 96)]
PRESENCE_FIELDS = ("statistic", "p_value", "n_exceed", "tested", "exposures", "reconstruction_errors", "null_exposures", "null_errors",
                   "null_statistics", "null_mean", "n_iterations", "converged", "null_n_iterations", "draws")
POWER_FIELDS = ("power", "detection_limit", "n_detected", "alt_mean", "planted_exposures", "alt_statistics", "alt_n_iterations", "alt_n_exceed",
                "alt_draws")


def case(K, V):
    """(counts, signatures, test, candidates): Poisson counts with totals 0, 1, 2, 257 and 100 000 on rows 0..4 (row 3 drawn from
    the last signature, a tested one with zeros); an (N, K) mask in which rows 5 and 6 do not hold test[0] and row 7 holds
    test[-1] alone.  For K > 2 every other set holds the dense signature 1."""
    rng = np.random.default_rng(2000 * K + V)
    X, W = refit_ref.poisson_catalogue(N, K, V=V, seed=80 + K, zero_heavy=2)
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
    C[5:7, test[0]] = K == 1
    C[7] = False
    C[7, test[-1]] = True
    return X, W, test, C


_results = {}


def run_of(K, V):
    """One call per case, shared by the tests that read it (none changes it)."""
    if (K, V) not in _results:
        X, W, test, C = case(K, V)
        _results[K, V] = (X, W, test, C, sal.signature_power(X, W, test, shares=SHARES, n_draws=B, n_alt_draws=A, alpha=ALPHA, seed=SEED, candidates=C,
                                                             keep_draws=True, **FIT))
    return _results[K, V]


def solve(X, W, C):
    return sal.assign_signatures(X, W, candidates=C, required=C, **FIT)


def without(C, s):
    C0 = C.copy()
    C0[:, s] = False
    return C0


@pytest.mark.parametrize("K,V", CASES)
def test_presence_part_is_the_presence_test(K, V):
    X, W, test, C, res = run_of(K, V)
    want = sal.signature_presence_test(X, W, test, n_draws=B, seed=SEED, candidates=C, keep_draws=True, **FIT)
    for name in PRESENCE_FIELDS:
        got, exp = getattr(res.presence, name), getattr(want, name)
        assert got.dtype == exp.dtype and np.array_equal(got, exp, equal_nan=True), name
    assert res.presence.test == want.test and np.array_equal(res.presence.candidates, want.candidates)


@pytest.mark.parametrize("K,V", CASES)
def test_untested_pairs_and_shapes(K, V):
    X, W, test, C, res = run_of(K, V)
    S, L = len(test), len(SHARES)
    tested = presence_ref.tested_pairs(C, test)
    assert np.array_equal(res.presence.tested, tested) and res.max_exceed == 1 and np.array_equal(res.shares, np.array(SHARES))
    if K == 1:
        assert not tested.any()
    else:
        assert not tested[5:7, 0].any() and tested[5:7, 1].all() and not tested[7].any() and tested[:5].all()
    assert res.power.shape == (L, N, S) and np.array_equal(np.isnan(res.power), np.broadcast_to(~tested, (L, N, S)))
    assert res.alt_mean.shape == (L, N, S) and np.array_equal(np.isnan(res.alt_mean), np.broadcast_to(~tested, (L, N, S)))
    assert res.alt_statistics.shape == (L, A, N, S) and np.array_equal(np.isnan(res.alt_statistics), np.broadcast_to(~tested, (L, A, N, S)))
    assert res.planted_exposures.shape == (L, N, S, K) and np.array_equal(np.isnan(res.planted_exposures).all(axis=3), np.broadcast_to(~tested, (L, N, S)))
    assert not np.isnan(res.planted_exposures[:, tested]).any()
    assert res.alt_draws.shape == (L, A, N, S, V) and not res.alt_draws[:, :, ~tested].any()
    assert res.alt_n_iterations.shape == (L, A, N, S, 2) and not res.alt_n_iterations[:, :, ~tested].any()
    assert res.alt_n_exceed.shape == (L, A, N, S) and not res.alt_n_exceed[:, :, ~tested].any() and not res.n_detected[:, ~tested].any()
    assert res.detection_limit.shape == (N, S) and np.isnan(res.detection_limit[~tested]).all()
    assert res.n_detected.dtype == np.int32 and res.alt_n_exceed.dtype == np.int32 and res.alt_n_iterations.dtype == np.int32


@pytest.mark.parametrize("K,V", CASES[1:])
def test_planted_exposures_equal_the_replica(K, V):
    X, W, test, C, res = run_of(K, V)
    H0 = res.presence.null_exposures
    assert np.array_equal(res.planted_exposures, ref.plant_all(H0, test, SHARES), equal_nan=True)
    assert np.array_equal(res.planted_exposures[0], H0, equal_nan=True)  # share 0: h0 bit for bit
    for j, s in enumerate(test):
        rows = np.flatnonzero(res.presence.tested[:, j])
        assert (res.planted_exposures[0, rows, j, s] == 0.0).all() and (res.planted_exposures[1, rows[X[rows].sum(axis=1) > 0], j, s] > 0.0).all()


@pytest.mark.parametrize("K,V", CASES[1:])
def test_alternative_draws_equal_the_replica(K, V):
    X, W, test, C, res = run_of(K, V)
    tested, totals = res.presence.tested, X.sum(axis=1)
    want = ref.draws_from(res.planted_exposures, refit_ref.normalize(W), totals, test, tested, A, SEED)
    assert np.array_equal(res.alt_draws, want)
    assert np.array_equal(res.alt_draws.sum(axis=4), np.broadcast_to(np.where(tested, totals[:, None], 0.0), (len(SHARES), A, N, len(test))))
    # another stream than the null draws'; the planted signature shows; draws differ in a
    assert not np.array_equal(res.alt_draws[0, :, 4], res.presence.draws[:A, 4])
    assert not np.array_equal(res.alt_draws[0, 0, 4, 0], res.alt_draws[1, 0, 4, 0]) and not np.array_equal(res.alt_draws[1, 0, 4, 0], res.alt_draws[1, 1, 4, 0])


@pytest.mark.parametrize("K,V", CASES[1:])
def test_alternative_statistics_are_the_two_solves_of_the_kept_draws(K, V):
    X, W, test, C, res = run_of(K, V)
    for j, s in enumerate(test):
        rows = np.flatnonzero(res.presence.tested[:, j])
        for l in range(len(SHARES)):
            for a in range(A):
                drawn = res.alt_draws[l, a, rows, j]
                alt, null = solve(drawn, W, C[rows]), solve(drawn, W, without(C[rows], s))
                assert np.array_equal(res.alt_statistics[l, a, rows, j], null.reconstruction_errors - alt.reconstruction_errors), (s, l, a)
                assert np.array_equal(res.alt_n_iterations[l, a, rows, j], np.stack([alt.n_iterations, null.n_iterations], axis=1)), (s, l, a)


@pytest.mark.parametrize("K,V", CASES[1:])
def test_reduction(K, V):
    _, _, _, _, res = run_of(K, V)
    tested = res.presence.tested
    e, n_detected, mean = ref.reduce_alt(res.presence.null_statistics, res.alt_statistics, ref.max_exceed(ALPHA, B))
    assert np.array_equal(res.alt_n_exceed, e) and np.array_equal(res.n_detected, n_detected) and np.array_equal(res.alt_mean, mean, equal_nan=True)
    power = ref.power_of(n_detected, A, tested)
    assert np.array_equal(res.power, power, equal_nan=True)
    assert np.array_equal(res.detection_limit, ref.detection_limit(SHARES, power, 0.8), equal_nan=True)
    # "detected" is "the presence test would have given p <= alpha against this null"
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res.n_detected[:, tested], ((1 + res.alt_n_exceed) / (B + 1) <= ALPHA).sum(axis=1)[:, tested])
    assert 1 < np.unique(res.alt_n_exceed[:, :, tested]).size
    for key in ("plant_s", "alt_draw_s", "alt_solve_s", "power_reduce_s", "alt_presence_kernel_ms", "total_s"):
        assert res.timings[key] >= 0.0
    assert res.timings["n_alt_chunks"] == 1 and res.presence.timings["n_chunks"] == 1


def test_a_level_does_not_depend_on_the_other_shares_or_on_the_number_of_draws():
    X, W, test, C, both = run_of(17, 96)
    wide = sal.signature_power(X, W, test, shares=SHARES, n_draws=B, n_alt_draws=4, alpha=ALPHA, seed=SEED, candidates=C, keep_draws=True, **FIT)
    one = sal.signature_power(X, W, test, shares=[0.25], n_draws=B, n_alt_draws=2, alpha=ALPHA, seed=SEED, candidates=C, keep_draws=True, **FIT)
    for name in ("alt_statistics", "alt_n_iterations", "alt_n_exceed", "alt_draws"):
        assert np.array_equal(getattr(one, name)[0], getattr(wide, name)[1, :2], equal_nan=True), name
        assert np.array_equal(getattr(one, name)[0], getattr(both, name)[1], equal_nan=True), name
    assert np.array_equal(one.planted_exposures[0], wide.planted_exposures[1], equal_nan=True)
    for name in ("n_detected", "alt_mean", "power"):
        assert np.array_equal(getattr(one, name)[0], getattr(both, name)[1], equal_nan=True), name
    for name in PRESENCE_FIELDS:
        assert np.array_equal(getattr(one.presence, name), getattr(both.presence, name), equal_nan=True), name


def test_chunks_give_the_same_bits():
    X, W, test, C, whole = run_of(3, 7)
    pairs = int(whole.presence.tested.sum())
    for per_chunk, n_chunks, n_alt_chunks in ((1, 3, 4), (2, 2, 2)):
        res = sal.signature_power(X, W, test, shares=SHARES, n_draws=B, n_alt_draws=A, alpha=ALPHA, seed=SEED, candidates=C, keep_draws=True,
                                  chunk_bytes=per_chunk * pairs * 7 * 8, **FIT)
        assert res.presence.timings["n_chunks"] == n_chunks and res.timings["n_alt_chunks"] == n_alt_chunks
        for name in PRESENCE_FIELDS:
            assert np.array_equal(getattr(res.presence, name), getattr(whole.presence, name), equal_nan=True), (per_chunk, name)
        for name in POWER_FIELDS:
            assert np.array_equal(getattr(res, name), getattr(whole, name), equal_nan=True), (per_chunk, name)
    assert sal.signature_power(X, W, test, shares=SHARES, n_draws=B, n_alt_draws=A, alpha=ALPHA, **FIT).alt_draws is None


def test_calibration():
    """The 64 null samples of tests/test_power_host.py at the defaults' convergence rule, under the same two conditions (the
    device's solves stop on their own tests, the replica's at a fixed step count: bounds, not equalities).  The device gives 145
    detections of 2 560 at share 0 (the cap is 154), mean power 0.0566 / 1.0 / 1.0, a detection limit of 0.05 for all 64."""
    X, S, s = presence_ref.calibration_samples()
    res = sal.signature_power(X[:64], S, [s], shares=(0.0, 0.05, 0.2), n_draws=39, n_alt_draws=40, alpha=0.05, target_power=0.8, seed=0)
    pooled = int(res.n_detected[0].sum())
    mean_power = res.power.mean(axis=(1, 2))
    print(f"max_exceed {res.max_exceed}; pooled detections at share 0: {pooled} of {64 * 40}; mean power per share {mean_power}; "
          f"detection limits {np.unique(res.detection_limit, return_counts=True)}; timings {res.timings}")
    assert res.presence.tested.all() and res.max_exceed == 1
    assert pooled <= ref.binomial_cap(64 * 40, 0.05, 0.01)
    assert mean_power[2] >= 0.8


def test_errors_through_the_c_abi():
    lib = _lib.load_with_device()
    p = _lib.pointer
    X = np.ones((4, 10))
    W = np.full((3, 10), 0.1)
    t = np.array([0, 1], dtype=np.int32)
    f64, i32 = (lambda *shape: np.empty(shape)), (lambda *shape: np.empty(shape, dtype=np.int32))
    Bn, Ln, An = 5, 65, 2
    presence = (np.empty((4, 2), dtype=np.uint8), f64(4, 2), i32(4, 2), f64(4, 2), f64(4, 3), f64(4), f64(4, 2, 3), f64(4, 2), i32(4, 2, 2), i32(4, 2, 2),
                f64(Bn, 4, 2), i32(Bn, 4, 2, 2))
    power = (f64(Ln, 4, 2, 3), f64(Ln, An, 4, 2), i32(Ln, An, 4, 2, 2), i32(Ln, An, 4, 2), i32(Ln, 4, 2), f64(Ln, 4, 2))

    def call(shares, n_alt_draws=An, max_exceed=1):
        sh = np.array(shares, dtype=np.float64)
        return lib.salnmf_signature_power(0, p(X), 4, 10, p(W), 3, p(t), 2, None, Bn, 0, 10, 20, 10, 1e-7, 0, p(sh), sh.size, n_alt_draws, max_exceed,
                                          *(p(a) for a in presence), None, *(p(a) for a in power), None, None)

    assert call([0.0, 1.0]) == 1 and "share 1 must be finite and in [0, 1), got 1" in _lib.last_error()
    assert call([0.2, 0.1]) == 1 and "shares must be strictly ascending: share 1 is 0.1 after 0.2" in _lib.last_error()
    assert call(list(np.arange(65) / 100.0)) == 1 and "n_shares must be in [1, 64], got 65" in _lib.last_error()
    assert call([0.0, 0.5], n_alt_draws=0) == 1 and "n_alt_draws must be in [1, 65536], got 0" in _lib.last_error()
    assert call([0.0, 0.5], max_exceed=Bn + 1) == 1 and "max_exceed must be in [0, 5], got 6" in _lib.last_error()
    assert call([0.0, 0.5]) == 0 and presence[0].all() and np.isfinite(power[1][:2]).all() and (power[4][:2] <= An).all()
