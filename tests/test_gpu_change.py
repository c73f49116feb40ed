"""``sal.exposure_change_test`` on the device: the three observed fits against the three
``sal.assign_signatures(candidates=C, required=C)`` calls of the contract, the null divergences against the replica's longdouble
evaluation at the device's own pooled exposures (tests/_change_ref.py; tolerance 16 x the float64 spread measured on the CPU on
these inputs, tests/test_change_host.py), the draws against the replica from the device's own pooled exposures, the reduction
against its stated rules, and the calibration pairs of tests/test_change_host.py.  ``np.array_equal`` unless stated."""

import numpy as np
import pytest

import _change_ref as ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import _lib

pytestmark = pytest.mark.gpu

N = ref.GPU_N
B = 3
SEED = 12345678901234567
FIT = ref.GPU_FIT
CASES = ref.GPU_CASES
G_TOL = 16 * ref.G_SPREAD  # of g_a and g_b, relative to the row's sum_v |x log(x / p)| + x + p
EPS64 = float(np.finfo(np.float64).eps)
NAMES = ("statistic", "p_value", "n_exceed", "tested", "null_mean", "exposures_a", "exposures_b", "pooled_exposures", "errors", "null_errors",
         "n_iterations", "converged", "shares_a", "shares_b", "share_difference", "null_statistics", "null_n_iterations", "draws")

_results = {}


def run_of(K, V):
    """One call per case, shared by the tests that read it (none changes it)."""
    if (K, V) not in _results:
        Xa, Xb, W, C = ref.gpu_case(K, V)
        _results[K, V] = (Xa, Xb, W, C, sal.exposure_change_test(Xa, Xb, W, n_draws=B, seed=SEED, candidates=C, keep_draws=True, **FIT))
    return _results[K, V]


def solve(X, W, A):
    """The contract's solve on the sets A, by the product's own assignment call."""
    return sal.assign_signatures(X, W, candidates=A, required=A, **FIT)


def clipped_sum(Xa, Xb):
    return np.maximum(Xa, ref.EPSILON) + np.maximum(Xb, ref.EPSILON)


def statistic_bounds(Xa, Xb, W, H0, fa, fb):
    """(statistic from the longdouble g_a, g_b and the given f_a, f_b; its tolerance): G_TOL on each null divergence, and four
    float64 roundings -- the three of the composition and the device's own product c P -- on numbers no larger than the scales."""
    ga, gb, sa, sb = ref.null_divergences(Xa, Xb, W, H0, dtype=np.longdouble)
    want = ((ga - fa) + (gb - fb)).astype(np.float64)
    return want, (G_TOL + 4 * EPS64) * (sa + sb).astype(np.float64)


@pytest.mark.parametrize("K,V", CASES)
def test_untested_pairs_and_shapes(K, V):
    Xa, Xb, W, C, res = run_of(K, V)
    want = ref.tested_pairs(Xa, Xb, C)
    assert res.tested.dtype == bool and np.array_equal(res.tested, want) and np.array_equal(res.candidates, C)
    assert not want.any() if K == 1 else (not want[[0, 5, 9]].any() and want[1:5].all())
    for name in ("statistic", "p_value", "null_mean"):
        assert getattr(res, name).shape == (N,) and np.array_equal(np.isnan(getattr(res, name)), ~want), name
    for name, width in (("exposures_a", K), ("exposures_b", K), ("pooled_exposures", K), ("errors", 3), ("null_errors", 2), ("shares_a", K),
                        ("shares_b", K), ("share_difference", K)):
        got = getattr(res, name)
        assert got.shape == (N, width) and np.array_equal(np.isnan(got).all(axis=1), ~want) and not np.isnan(got[want]).any(), name
    assert res.null_statistics.shape == (B, N) and np.array_equal(np.isnan(res.null_statistics), np.broadcast_to(~want, (B, N)))
    assert res.draws.shape == (B, N, 2, V) and not res.draws[:, ~want].any()
    assert res.n_iterations.shape == (N, 3) and res.null_n_iterations.shape == (B, N, 3)
    assert not res.n_exceed[~want].any() and not res.n_iterations[~want].any() and not res.null_n_iterations[:, ~want].any()
    assert res.n_iterations.dtype == np.int32 and res.n_exceed.dtype == np.int32 and res.converged.dtype == bool and not res.converged[~want].any()


@pytest.mark.parametrize("K,V", CASES[1:])
def test_observed_fits_are_the_three_masked_solves(K, V):
    Xa, Xb, W, C, res = run_of(K, V)
    rows = np.flatnonzero(res.tested)
    for i, (X, H) in enumerate(((Xa, res.exposures_a), (Xb, res.exposures_b), (clipped_sum(Xa, Xb), res.pooled_exposures))):
        fit = solve(X[rows], W, C[rows])
        assert np.array_equal(H[rows], fit.exposures), i
        assert np.array_equal(res.errors[rows, i], fit.reconstruction_errors), i
        assert np.array_equal(res.n_iterations[rows, i], fit.n_iterations) and np.array_equal(res.converged[rows, i], fit.converged), i
        assert (H[rows][~C[rows]] == 0.0).all()
    if V > 1:  # (with one feature every solve sits at its fixed point after one step)
        assert 1 < np.unique(res.n_iterations[rows]).size  # problems of one tile stop at different tests
        assert not res.converged[rows].all() and res.converged[rows].any()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res.shares_a[rows], res.exposures_a[rows] / res.exposures_a[rows].sum(axis=1, keepdims=True))
        assert np.array_equal(res.shares_b[rows], res.exposures_b[rows] / res.exposures_b[rows].sum(axis=1, keepdims=True))
    assert np.array_equal(res.share_difference[rows], res.shares_b[rows] - res.shares_a[rows])


@pytest.mark.parametrize("K,V", CASES[1:])
def test_statistic_and_null_divergences(K, V):
    Xa, Xb, W, C, res = run_of(K, V)
    rows = np.flatnonzero(res.tested)
    e, g = res.errors[rows], res.null_errors[rows]
    assert np.array_equal(res.statistic[rows], (g[:, 0] - e[:, 0]) + (g[:, 1] - e[:, 1]))
    ga, gb, sa, sb = ref.null_divergences(Xa[rows], Xb[rows], W, res.pooled_exposures[rows], dtype=np.longdouble)
    dev = max(float((np.abs(g[:, 0] - ga) / sa).max()), float((np.abs(g[:, 1] - gb) / sb).max()))
    print(f"K = {K}, V = {V}: null divergences within {dev:.3g} of the longdouble evaluation (tolerance {G_TOL:.3g})")
    assert dev <= G_TOL


@pytest.mark.parametrize("K,V", CASES[1:])
def test_draws_equal_the_replica(K, V):
    Xa, Xb, W, C, res = run_of(K, V)
    want = ref.draws_from(res.pooled_exposures, refit_ref.normalize(W), Xa.sum(axis=1), Xb.sum(axis=1), res.tested, B, SEED)
    assert np.array_equal(res.draws, want)
    totals = np.where(res.tested[:, None], np.stack([Xa.sum(axis=1), Xb.sum(axis=1)], axis=1), 0.0)
    assert np.array_equal(res.draws.sum(axis=3), np.broadcast_to(totals, (B, N, 2)))
    if V > 1:  # (with one feature every draw is the row's total)
        assert not np.array_equal(res.draws[0, 3, 0], res.draws[1, 3, 0]) and not np.array_equal(res.draws[0, 6, 0], res.draws[0, 6, 1])


@pytest.mark.parametrize("K,V", CASES[1:])
def test_null_statistics_are_the_procedure_on_the_kept_draws(K, V):
    Xa, Xb, W, C, res = run_of(K, V)
    rows = np.flatnonzero(res.tested)
    worst = 0.0
    for b in range(B):
        da, db = res.draws[b, rows, 0], res.draws[b, rows, 1]
        a, bb, pooled = solve(da, W, C[rows]), solve(db, W, C[rows]), solve(clipped_sum(da, db), W, C[rows])
        assert np.array_equal(res.null_n_iterations[b, rows], np.stack([a.n_iterations, bb.n_iterations, pooled.n_iterations], axis=1)), b
        want, tol = statistic_bounds(da, db, W, pooled.exposures, a.reconstruction_errors, bb.reconstruction_errors)
        worst = max(worst, float((np.abs(res.null_statistics[b, rows] - want) / tol).max()))
    print(f"K = {K}, V = {V}: null statistics at {worst:.3g} of their tolerance")
    assert worst <= 1.0


@pytest.mark.parametrize("K,V", CASES[1:])
def test_reduction(K, V):
    _, _, _, _, res = run_of(K, V)
    n_exceed, mean, p = ref.reduce_null(res.statistic, res.null_statistics)
    assert np.array_equal(res.n_exceed, n_exceed) and np.array_equal(res.null_mean, mean, equal_nan=True) and np.array_equal(res.p_value, p, equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res.n_exceed, (res.null_statistics >= res.statistic).sum(axis=0))
    assert np.array_equal(res.p_value[res.tested], (1 + res.n_exceed[res.tested]) / (B + 1))
    for key in ("draw_s", "solve_s", "reduce_s", "total_s", "change_kernel_ms"):
        assert res.timings[key] >= 0.0
    assert res.timings["n_chunks"] == 1


def test_a_pair_does_not_depend_on_the_number_of_draws_or_on_the_other_pairs():
    Xa, Xb, W, _ = ref.gpu_case(17, 96)
    eight = sal.exposure_change_test(Xa, Xb, W, n_draws=8, seed=3, keep_draws=True, **FIT)
    four = sal.exposure_change_test(Xa, Xb, W, n_draws=4, seed=3, keep_draws=True, **FIT)
    assert eight.candidates is None and np.array_equal(eight.tested, ref.tested_pairs(Xa, Xb, np.ones((N, 17), dtype=bool)))
    for name in ("statistic", "exposures_a", "exposures_b", "pooled_exposures", "errors", "null_errors", "n_iterations", "converged"):
        assert np.array_equal(getattr(four, name), getattr(eight, name), equal_nan=True), name
    for name in ("null_statistics", "null_n_iterations", "draws"):
        assert np.array_equal(getattr(four, name), getattr(eight, name)[:4], equal_nan=True), name  # B = 4 against the first 4 of B = 8
    # a row subset against the full call: the fits do not see n; the draws do, so the rows that keep their index keep everything
    head = sal.exposure_change_test(Xa[:20], Xb[:20], W, n_draws=4, seed=3, keep_draws=True, **FIT)
    for name in NAMES:
        full = getattr(four, name)
        assert np.array_equal(getattr(head, name), full[:, :20] if name in ("null_statistics", "null_n_iterations", "draws") else full[:20], equal_nan=True), name
    moved = sal.exposure_change_test(Xa[[7, 3, 30]], Xb[[7, 3, 30]], W, n_draws=4, seed=3, **FIT)
    for name in ("statistic", "exposures_a", "exposures_b", "pooled_exposures", "errors", "null_errors", "n_iterations", "converged"):
        assert np.array_equal(getattr(moved, name), getattr(four, name)[[7, 3, 30]]), name
    assert not np.array_equal(sal.exposure_change_test(Xa, Xb, W, n_draws=1, seed=4, keep_draws=True, **FIT).draws[0], four.draws[0])


def test_chunks_give_the_same_bits():
    Xa, Xb, W, C, whole = run_of(3, 7)
    pairs = int(whole.tested.sum())
    for per_chunk, n_chunks in ((1, 3), (2, 2)):
        res = sal.exposure_change_test(Xa, Xb, W, n_draws=B, seed=SEED, candidates=C, keep_draws=True, chunk_bytes=per_chunk * pairs * 2 * 7 * 8, **FIT)
        assert res.timings["n_chunks"] == n_chunks
        for name in NAMES:
            assert np.array_equal(getattr(res, name), getattr(whole, name), equal_nan=True), (per_chunk, name)
    assert sal.exposure_change_test(Xa, Xb, W, n_draws=2, **FIT).draws is None


def test_changed_shares_and_calibration():
    """The 64 + 8 pairs of tests/test_change_host.py at the defaults' convergence rule, under the same two conditions (the
    device's solves stop on their own tests, the replica's at a fixed step count: bounds, not equalities).  The device gives 4 of
    64 at or below 0.05, all 8 planted pairs at n_exceed 0, their statistics 45 to 106 times the largest null one."""
    Xa, Xb, S = ref.calibration_pairs()
    res = sal.exposure_change_test(Xa, Xb, S, n_draws=39, seed=0)
    null = res.p_value[:64]
    ratio = res.statistic[64:] / res.null_statistics[:, 64:].max(axis=0)
    print(f"null pairs: {int((null <= 0.05).sum())} of 64 at or below 0.05, mean p {null.mean():.3f}; planted n_exceed {res.n_exceed[64:]}, "
          f"statistic / largest null {ratio.min():.1f} .. {ratio.max():.1f}; iterations {res.n_iterations.min()}..{res.n_iterations.max()}, "
          f"null {res.null_n_iterations.min()}..{res.null_n_iterations.max()}; smallest statistic {res.statistic.min():.3g}")
    assert res.tested.all()
    assert (null <= 0.05).sum() <= 8
    assert np.array_equal(res.n_exceed[64:], np.zeros(8, dtype=np.int32))
    assert np.array_equal(res.p_value[64:], np.full(8, 1 / 40))


def test_errors_through_the_c_abi():
    lib = _lib.load_with_device()
    p = _lib.pointer
    X = np.ones((4, 10))
    out = dict(tested=np.empty(4, dtype=np.uint8), stat=np.empty(4), exceed=np.empty(4, dtype=np.int32), mean=np.empty(4), Ha=np.empty((4, 97)),
               Hb=np.empty((4, 97)), H0=np.empty((4, 97)), err=np.empty((4, 3)), err0=np.empty((4, 2)), nit=np.empty((4, 3), dtype=np.int32),
               conv=np.empty((4, 3), dtype=np.int32), stat_b=np.empty((5, 4)), nit_b=np.empty((5, 4, 3), dtype=np.int32))

    def call(W, n_draws, Xa=X, Xb=X, max_it=20):
        return lib.salnmf_exposure_change(0, p(Xa), Xa.shape[0], Xa.shape[1], p(Xb), Xb.shape[0], Xb.shape[1], p(W), W.shape[0], None, n_draws, 0, 10,
                                          max_it, 10, 1e-7, 0, *(p(a) for a in out.values()), None, None)

    W = np.full((3, 10), 0.1)
    half = np.where(np.arange(40).reshape(4, 10) == 12, 0.5, X)
    assert call(np.full((97, 10), 0.1), 5) == 1 and "n_signatures must be in [1, 96], got 97" in _lib.last_error()
    assert call(W, 0) == 1 and "n_draws must be in [1, 65536], got 0" in _lib.last_error()
    assert call(W, 5, Xb=np.ones((3, 10))) == 1 and "the shapes must agree, got 4 x 10 and 3 x 10" in _lib.last_error()
    assert call(W, 5, Xb=np.ones((4, 9))) == 1 and "the shapes must agree, got 4 x 10 and 4 x 9" in _lib.last_error()
    assert call(W, 5, Xa=half) == 1 and "integer counts below 2^32: row 1, column 2 holds 0.5" in _lib.last_error()
    assert call(W, 5, Xb=half) == 1 and "integer counts below 2^32: row 1, column 2 holds 0.5" in _lib.last_error()
    assert call(W, 5, max_it=25) == 1 and "max_iterations must be a multiple of conv_test_freq, got 25 and 10" in _lib.last_error()
    assert call(W, 5) == 0 and out["tested"].all() and np.isfinite(out["stat"]).all() and np.isfinite(out["stat_b"]).all()
