"""``sal.profile_likelihood`` and ``sal.exposure_intervals`` on the device, on the cases of
tests/test_gpu_presence.py: the frozen solve at 0 against the presence test and the masked assignment call, bit for bit; the
profile against the host replica (tests/_profile_ref.py); a pair against its tile neighbours; every trial of the search against
the primitive and the whole search against the replica's rule fed with the device's own profile values -- ``np.array_equal``
--; and the coverage samples of tests/test_profile_host.py."""

import numpy as np
import pytest

import _assign_masks_ref as masks_ref
import _profile_ref as ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import _lib
from test_gpu_presence import FIT, N, case

pytestmark = pytest.mark.gpu

CASES = [(3, 7), (17, 96), (96, 96)]
DELTA = 1.92
J, E = 5, 40
STEPS = dict(min_iterations=20, max_iterations=20, conv_test_freq=10)  # every solve is 20 steps long: the replica comparison

_runs = {}


def run_of(K, V):
    """One interval call and one replica run per case, shared by the tests that read them (none changes them)."""
    if (K, V) not in _runs:
        X, W, test, C = case(K, V)
        got = sal.exposure_intervals(X, W, test, candidates=C, max_kl_increase=DELTA, n_bisections=J, max_expansions=E, keep_trace=True, **FIT)
        want = ref.intervals(X, W, test, candidates=C, max_kl_increase=DELTA, n_bisections=J, max_expansions=E, **FIT)
        _runs[K, V] = (X, W, test, C, got, want)
    return _runs[K, V]


def grid_of(K):
    """(N, S, 4) values: 0, one below most estimates, two above; scaled by the sample so that pairs differ."""
    S = 1 if K == 1 else 2
    return np.broadcast_to(np.array([0.0, 0.5, 30.0, 4000.0])[None, None, :] * (1.0 + np.arange(N) % 3)[:, None, None], (N, S, 4)).copy()


@pytest.mark.parametrize("K,V", CASES)
def test_the_profile_at_zero_is_the_presence_statistic(K, V):
    X, W, test, C = case(K, V)
    S = len(test)
    got = sal.profile_likelihood(X, W, test, [0.0], candidates=C, **FIT)
    pres = sal.signature_presence_test(X, W, test, n_draws=1, candidates=C, **FIT)
    want = ref.presence_ref.tested_pairs(C, test)
    assert got.tested.dtype == bool and np.array_equal(got.tested, want) and np.array_equal(got.tested, pres.tested) and got.test == tuple(test)
    assert got.profile.shape == (N, S, 1) and got.errors.shape == (N, S, 1) and got.n_iterations.shape == (N, S, 1) and got.converged.shape == (N, S, 1)
    assert np.array_equal(np.isnan(got.profile[..., 0]), ~want) and np.array_equal(np.isnan(got.errors[..., 0]), ~want)
    assert not got.n_iterations[~want].any() and not got.converged[~want].any() and got.profile_exposures is None
    assert not want[5:9, 0].any() and want[5:9, 1].all() and not want[9].any() and not want[10].any() and want[:5].all()
    assert np.array_equal(got.profile[..., 0], pres.statistic, equal_nan=True)
    assert np.array_equal(got.errors[..., 0], pres.null_errors, equal_nan=True)
    assert np.array_equal(got.n_iterations[..., 0], pres.n_iterations[..., 1]) and np.array_equal(got.converged[..., 0], pres.converged[..., 1])
    assert np.array_equal(got.exposures, pres.exposures, equal_nan=True)
    assert np.array_equal(got.reconstruction_errors, pres.reconstruction_errors, equal_nan=True)
    rows = np.flatnonzero(want.any(axis=1))
    alt = sal.assign_signatures(X[rows], W, candidates=C[rows], required=C[rows], **FIT)
    assert np.array_equal(got.exposures[rows], alt.exposures) and np.array_equal(got.reconstruction_errors[rows], alt.reconstruction_errors)
    for j, s in enumerate(test):
        rows = np.flatnonzero(want[:, j])
        C0 = C[rows].copy()
        C0[:, s] = False
        null = sal.assign_signatures(X[rows], W, candidates=C0, required=C0, **FIT)
        assert np.array_equal(got.errors[rows, j, 0], null.reconstruction_errors) and np.array_equal(got.n_iterations[rows, j, 0], null.n_iterations)
    assert 1 < np.unique(got.n_iterations[want]).size  # problems of one tile stop at different tests
    # non-integer counts are taken: nothing is drawn
    assert np.isfinite(sal.profile_likelihood(X + 0.25, W, test, [0.0, 1.0], candidates=C, **FIT).profile[want]).all()


@pytest.mark.parametrize("K,V", CASES)
def test_the_frozen_entry_and_the_replica(K, V):
    """At 20-step solves the device's f and exposures against the float64 replica.  The tolerance is the one
    tests/test_gpu_assign_masks.py holds the device to against its replica: 16 x the spread of the float64 feature orders about
    the longdouble replica (``_assign_masks_ref.H_SPREAD`` / ``F_SPREAD``), |dH| / max(H, EPSILON) on the free support and |df|
    relative to the row's sum_v |x log(x / wh)| + x + wh; the profile is a difference of two such f."""
    X, W, test, C = case(K, V)
    values = grid_of(K)
    got = sal.profile_likelihood(X, W, test, values, candidates=C, keep_exposures=True, **STEPS)
    want = ref.profile(X, W, test, values, candidates=C, **STEPS)
    t = got.tested
    assert np.array_equal(t, want.tested) and got.profile_exposures.shape == (N, len(test), 4, K)
    assert np.array_equal(got.n_iterations[t], np.full((int(t.sum()), 4), 20))
    worst_h = worst_f = worst_g = 0.0
    for j, s in enumerate(test):
        rows = np.flatnonzero(t[:, j])
        H = got.profile_exposures[rows, j]
        assert np.array_equal(H[:, :, s], values[rows, j])  # the frozen entry is exactly c
        assert (H[np.broadcast_to(~C[rows][:, None, :], H.shape)] == 0.0).all()  # exact zeros off the set
        assert np.isnan(got.profile_exposures[~t[:, j], j]).all()
        free = C[rows].copy()
        free[:, s] = False
        for i in range(4):
            Hw = want.profile_exposures[rows, j, i]
            scale = masks_ref.row_scale(X[rows], refit_ref.normalize(W), Hw)
            worst_h = max(worst_h, float((np.abs(H[:, i] - Hw) / np.maximum(Hw, ref.EPSILON))[free].max()))
            worst_f = max(worst_f, float((np.abs(got.errors[rows, j, i] - want.errors[rows, j, i]) / scale).max()))
            worst_g = max(worst_g, float((np.abs(got.profile[rows, j, i] - want.profile[rows, j, i]) / scale).max()))
    print(f"K = {K}: |dH| / H {worst_h:.3g} (bound {16 * masks_ref.H_SPREAD:.3g}), |df| / scale {worst_f:.3g} (bound {16 * masks_ref.F_SPREAD:.3g}), "
          f"|dg| / scale {worst_g:.3g}")
    assert worst_h <= 16 * masks_ref.H_SPREAD
    assert worst_f <= 16 * masks_ref.F_SPREAD
    assert worst_g <= 2 * 16 * masks_ref.F_SPREAD


def test_a_pair_does_not_depend_on_its_tile_neighbours():
    X, W, test, C = case(17, 96)
    values = [0.0, 3.0, 250.0, 1e5, 0.125, 7.0, 7.0, 1.0, 40.0]  # nine values: a run of eight and a run of one
    whole = sal.profile_likelihood(X, W, test, values, candidates=C, keep_exposures=True, **FIT)
    perm = np.random.default_rng(5).permutation(N)
    moved = sal.profile_likelihood(X[perm], W, test[::-1], values, candidates=C[perm], keep_exposures=True, **FIT)
    names = ("profile", "errors", "n_iterations", "converged", "profile_exposures")
    for name in names:
        assert np.array_equal(getattr(moved, name), getattr(whole, name)[perm][:, ::-1], equal_nan=True), name
    assert np.array_equal(whole.profile[..., 5], whole.profile[..., 6], equal_nan=True)
    for n in (0, 4, 7, 23, 39):
        alone = sal.profile_likelihood(X[n:n + 1], W, test, values[2:3], candidates=C[n:n + 1], keep_exposures=True, **FIT)
        for name in names:
            assert np.array_equal(getattr(alone, name)[0, :, 0], getattr(whole, name)[n, :, 2], equal_nan=True), (n, name)
    res = sal.exposure_intervals(X, W, test, candidates=C, n_bisections=J, keep_trace=True, **FIT)
    moved = sal.exposure_intervals(X[perm], W, test[::-1], candidates=C[perm], n_bisections=J, keep_trace=True, **FIT)
    for name in ("lower", "upper", "estimate", "bracketed", "n_trials", "statistic", "null_errors", "trace_values", "trace_profile"):
        assert np.array_equal(getattr(moved, name), getattr(res, name)[perm][:, ::-1], equal_nan=True), name


@pytest.mark.parametrize("K,V", CASES)
def test_the_search_is_the_rule_on_the_primitives_values(K, V):
    X, W, test, C, got, _ = run_of(K, V)
    S, T = len(test), E + J
    t = got.tested
    assert got.trace_values.shape == (N, S, 2, T) and got.trace_profile.shape == (N, S, 2, T) and got.n_trials.dtype == np.int32
    past = np.arange(T)[None, None, None, :] >= got.n_trials[..., None]
    assert np.array_equal(np.isnan(got.trace_values), past) and np.array_equal(np.isnan(got.trace_profile), past)
    for name in ("lower", "upper", "estimate", "statistic", "null_errors"):
        assert np.array_equal(np.isnan(getattr(got, name)), ~t), name
    assert not got.n_trials[~t].any() and not got.bracketed[~t].any()
    # every trial is the primitive at the trial's value
    values = np.where(past, 0.0, got.trace_values).reshape(N, S, 2 * T)
    prim = sal.profile_likelihood(X, W, test, values, candidates=C, **FIT)
    assert np.array_equal(prim.profile.reshape(N, S, 2, T)[~past], got.trace_profile[~past])
    pres = sal.signature_presence_test(X, W, test, n_draws=1, candidates=C, **FIT)
    assert np.array_equal(got.statistic, pres.statistic, equal_nan=True) and np.array_equal(got.null_errors, pres.null_errors, equal_nan=True)
    assert np.array_equal(got.exposures, pres.exposures, equal_nan=True) and np.array_equal(got.estimate[t], pres.exposures[:, test][t])
    # the whole search is the replica's rule fed with the device's own profile values
    for n, j in zip(*np.nonzero(t)):
        want = ref.replay(got.trace_profile[n, j], got.estimate[n, j], got.statistic[n, j], delta=DELTA, n_bisections=J, max_expansions=E)
        assert np.array_equal(got.trace_values[n, j], want.trace_values, equal_nan=True), (n, j)
        assert np.array_equal(got.n_trials[n, j], want.n_trials), (n, j)
        assert got.lower[n, j] == want.lower and got.upper[n, j] == want.upper and got.bracketed[n, j] == want.bracketed, (n, j)
    assert (got.lower[t] <= got.estimate[t]).all() and (got.estimate[t] <= got.upper[t]).all()
    assert got.timings["n_problems"] == int(t.sum()) + int((got.statistic[t] > DELTA).sum()) and got.timings["profile_kernel_ms"] > 0.0


@pytest.mark.parametrize("K,V", CASES)
def test_kinds_of_pair(K, V):
    X, W, test, C, got, want = run_of(K, V)
    t = want.tested
    # on the CPU replica first: the fixture holds every kind of pair
    assert (want.lower[t] == 0.0).any() and (want.n_trials[..., 0][t] == 0).any()  # lower end 0 without a trial
    assert (want.n_trials[..., 0][t] == J).any() and (want.lower[t] > 0.0).any()  # lower end searched
    assert (want.n_trials[:3, :, 1] - J > 1).all() and want.bracketed[t].all()  # more than one expansion: the totals 0, 1 and 2
    loose = ref.intervals(X[:5], W, test, candidates=C[:5], max_kl_increase=50.0, n_bisections=J, max_expansions=2, **FIT)
    assert (~loose.bracketed).any() and loose.bracketed.any()
    # then the device: the same kinds.  A lower end is searched exactly where removing the signature costs more than the threshold
    assert np.array_equal(t, got.tested)
    assert np.array_equal(got.n_trials[..., 0][t] == 0, got.statistic[t] <= DELTA) and (got.lower[t][got.statistic[t] <= DELTA] == 0.0).all()
    assert (got.n_trials[:3, :, 1] - J > 1).all()
    assert np.array_equal(got.n_trials[t], want.n_trials[t]) and np.array_equal(got.bracketed, want.bracketed)
    dev = sal.exposure_intervals(X[:5], W, test, candidates=C[:5], max_kl_increase=50.0, n_bisections=J, max_expansions=2, keep_trace=True, **FIT)
    assert np.array_equal(dev.bracketed, loose.bracketed) and np.array_equal(np.isinf(dev.upper), ~loose.bracketed)
    assert (dev.n_trials[..., 1][~dev.bracketed] == 2).all() and dev.trace_values.shape == (5, len(test), 2, 2 + J)
    assert np.array_equal(dev.n_trials, loose.n_trials) and np.array_equal(dev.n_trials[..., 0] == 0, dev.statistic <= 50.0)


@pytest.mark.parametrize("K,V", CASES)
def test_boundary(K, V):
    """``(lower == 0) == (statistic <= max_kl_increase)`` on the tested pairs, at the five bisections this file runs with.

    Five halvings of [0, estimate] alone do not give it: in the (17, 96) case sample 14, signature 0 has statistic 1.970 > 1.92 at
    an estimate of 13.57 and its profile crosses 1.92 at c = 0.131, below estimate / 2**5 = 0.424 (the five trials' profile values:
    0.386, 0.958, 1.390, 1.660, 1.810, all inside), and the outer end of [0, 0.424] is 0.0.  The rule therefore goes on halving
    while the bracket still starts at 0.0, up to the first trial outside: here two more trials, and lower = 0.106."""
    _, _, _, _, got, _ = run_of(K, V)
    t = got.tested
    off = t & ((got.lower == 0.0) != (got.statistic <= DELTA))
    for n, j in zip(*np.nonzero(off)):
        print(f"sample {n}, signature {j}: statistic {got.statistic[n, j]:.6g}, estimate {got.estimate[n, j]:.6g}, lower {got.lower[n, j]}, "
              f"lower-end trials {got.trace_values[n, j, 0, :J]} -> {got.trace_profile[n, j, 0, :J]}")
    assert np.array_equal(got.lower[t] == 0.0, got.statistic[t] <= DELTA)
    if (K, V) == (17, 96):
        assert got.n_trials[14, 0, 0] == J + 2 and got.lower[14, 0] == got.estimate[14, 0] / 2.0 ** (J + 2) and (got.n_trials[..., 0] > J).sum() == 1


def test_coverage_on_the_device():
    """The first 64 coverage samples of tests/test_profile_host.py at the default iteration arguments: the device's solves and
    the replica's stop on their own tests and agree to rounding, so the covered samples differ by at most 2."""
    X, S, truth = ref.coverage_samples()
    X, truth = X[:64], truth[:64]
    want = ref.intervals(X, S, [0, 3])
    got = sal.exposure_intervals(X, S, [0, 3])

    def covered(res):
        return (res.lower[:, 0] <= truth[:, 0]) & (truth[:, 0] <= res.upper[:, 0])

    print(f"covered: device {int(covered(got).sum())}, replica {int(covered(want).sum())} of 64; lower == 0 for the absent signature: device "
          f"{int((got.lower[:, 1] == 0.0).sum())}, replica {int((want.lower[:, 1] == 0.0).sum())}; profile kernel {got.timings['profile_kernel_ms']:.1f} ms, "
          f"{got.timings['n_problems']} problems")
    assert got.tested.all() and got.bracketed.all() and got.trace_values is None
    assert abs(int(covered(got).sum()) - int(covered(want).sum())) <= 2
    assert np.array_equal(got.n_trials[:, 1, 0] == 0, got.statistic[:, 1] <= 1.92) and (got.lower[:, 1][got.statistic[:, 1] <= 1.92] == 0.0).all()
    # (the ends move with the stop tests' rounding by far less than the last bracket, estimate / 2**16)
    assert np.allclose(got.lower, want.lower, rtol=1e-3, atol=0.5) and np.allclose(got.upper, want.upper, rtol=1e-3, atol=0.5)


def test_errors_through_the_c_abi():
    lib = _lib.load_with_device()
    p = _lib.pointer
    X = np.ones((4, 10))
    f64, i32, u8 = (lambda *s: np.empty(s)), (lambda *s: np.empty(s, dtype=np.int32)), (lambda *s: np.empty(s, dtype=np.uint8))

    def profile(W, test, values, per_pair=0, max_it=20):
        t, v = np.array(test, dtype=np.int32), np.array(values, dtype=np.float64)
        M = v.shape[-1]
        out = (u8(4, 2), f64(4, 2, M), f64(4, 2, M), i32(4, 2, M), i32(4, 2, M), None, f64(4, 97), f64(4))
        rc = lib.salnmf_profile_likelihood(0, p(X), 4, 10, p(W), W.shape[0], p(t), t.size, None, p(v), M, per_pair, 10, max_it, 10, 1e-7,
                                           *(a if a is None else p(a) for a in out), None)
        return rc, out

    def intervals(W, test, delta=1.92, n_bisections=3, max_expansions=5, max_it=20):
        t = np.array(test, dtype=np.int32)
        out = (u8(4, 2), f64(4, 2), f64(4, 2), f64(4, 2), u8(4, 2), i32(4, 2, 2), f64(4, 2), f64(4, 2), f64(4, 97), f64(4))
        rc = lib.salnmf_exposure_intervals(0, p(X), 4, 10, p(W), W.shape[0], p(t), t.size, None, delta, n_bisections, max_expansions, 10, max_it, 10, 1e-7,
                                           *(p(a) for a in out), None, None, None)
        return rc, out

    W = np.full((3, 10), 0.1)
    for call in (lambda **kw: profile(kw.pop("W", W), kw.pop("test", [0, 1]), [0.0, 1.0], **kw), lambda **kw: intervals(kw.pop("W", W), kw.pop("test", [0, 1]), **kw)):
        assert call(W=np.full((97, 10), 0.1))[0] == 1 and "n_signatures must be in [1, 96], got 97" in _lib.last_error()
        assert call(test=[0, 3])[0] == 1 and "tested signature 3 is not in [0, 3)" in _lib.last_error()
        assert call(test=[1, 1])[0] == 1 and "signature 1 is tested twice" in _lib.last_error()
        assert call(max_it=25)[0] == 1 and "max_iterations must be a multiple of conv_test_freq, got 25 and 10" in _lib.last_error()
    assert profile(W, [0, 1], [0.0, -1.0])[0] == 1 and "values must be finite and not negative: entry 1 holds -1" in _lib.last_error()
    assert profile(W, [0, 1], [np.inf])[0] == 1 and "values must be finite and not negative" in _lib.last_error()
    assert profile(W, [0, 1], np.zeros(4097))[0] == 1 and "n_values must be in [1, 4096], got 4097" in _lib.last_error()
    assert profile(W, [0, 1], [0.0], per_pair=2)[0] == 1 and "values_per_pair must be 0 or 1, got 2" in _lib.last_error()
    assert intervals(W, [0, 1], delta=-1.0)[0] == 1 and "max_kl_increase must be finite and not negative, got -1" in _lib.last_error()
    assert intervals(W, [0, 1], delta=np.nan)[0] == 1 and "max_kl_increase must be finite and not negative" in _lib.last_error()
    assert intervals(W, [0, 1], n_bisections=-1)[0] == 1 and "n_bisections must be in [0, 64], got -1" in _lib.last_error()
    assert intervals(W, [0, 1], max_expansions=0)[0] == 1 and "max_expansions must be in [1, 1000], got 0" in _lib.last_error()
    rc, out = profile(W, [0, 1], [0.0, 1.0])
    assert rc == 0 and out[0].all() and np.isfinite(out[1]).all() and (out[3] > 0).all()
    rc, out = intervals(W, [0, 1], n_bisections=0)
    assert rc == 0 and out[0].all() and (out[1] == 0.0).all() and np.isfinite(out[2]).all() and not out[5][..., 0].any()
