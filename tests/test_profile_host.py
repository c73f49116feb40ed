"""The profile likelihood's host side without a device: the replica (tests/_profile_ref.py) against its own contract -- the
frozen solve at 0 is the presence test's null solve, the search rule on analytic convex functions, convexity of the profile,
coverage of the 95 % interval --, every argument ``sal.profile_likelihood`` and ``sal.exposure_intervals`` refuse before they
touch a device, and the shapes they return."""

import math

import numpy as np
import pytest

import _presence_ref as presence_ref
import _profile_ref as ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import intervals as intervals_mod


def small_case(N=6, K=4, V=10, seed=0):
    return refit_ref.poisson_catalogue(N, K, V=V, seed=seed, mutations=(50, 400))


def test_the_frozen_solve_at_zero_is_the_presence_tests_null_solve():
    X, W = small_case(N=9, K=5, V=12, seed=3)
    C = np.random.default_rng(0).random((9, 5)) < 0.7
    C[:, [0, 1, 3]] = True
    for kw in (dict(min_iterations=20, max_iterations=60, conv_test_freq=10, tol=1e-5), dict(min_iterations=30, max_iterations=30, conv_test_freq=5)):
        for s in (0, 3):
            C0 = C.copy()
            C0[:, s] = False
            null = presence_ref.solve(X, W, C0, **kw)
            mine = ref.frozen_solve(X, W, C, s, 0.0, **kw)
            assert np.array_equal(mine.exposures, null.exposures) and np.array_equal(mine.reconstruction_errors, null.reconstruction_errors)
            assert np.array_equal(mine.n_iterations, null.n_iterations) and np.array_equal(mine.converged, null.converged)
            assert (mine.exposures[:, s] == 0.0).all() and (mine.exposures[~C] == 0.0).all()
    # and the whole calls agree: profile(values=[0]) is the presence statistic
    kw = dict(min_iterations=20, max_iterations=60, conv_test_freq=10, tol=1e-5)
    got = ref.profile(X, W, [0, 3], [0.0, 2.5], candidates=C, **kw)
    pres = presence_ref.presence(X, W, [0, 3], 1, candidates=C, steps=20)
    fixed = ref.profile(X, W, [0, 3], [0.0], candidates=C, min_iterations=20, max_iterations=20, conv_test_freq=10)
    assert np.array_equal(fixed.profile[..., 0], pres.statistic) and np.array_equal(fixed.exposures, pres.exposures)
    assert got.tested.all() and (got.profile_exposures[:, 0, 1, 0] == 2.5).all() and (got.profile_exposures[:, 1, 1, 3] == 2.5).all()
    assert (got.profile_exposures[np.broadcast_to(~C[:, None, None, :], got.profile_exposures.shape)] == 0.0).all()


def convex(root_lo, root_hi):
    """(estimate, g): a convex parabola with minimum 0 at the estimate, the middle, that crosses `delta` at root_lo and root_hi."""
    mid, half = 0.5 * (root_lo + root_hi), 0.5 * (root_hi - root_lo)
    return mid, lambda c, delta=1.92: delta * ((c - mid) / half) ** 2


@pytest.mark.parametrize("root_lo,root_hi", [(3.0, 11.0), (0.37, 0.91), (1e3, 1.7e3), (120.0, 9000.0)])
def test_search_rule_brackets_the_roots(root_lo, root_hi):
    delta = 1.92
    est, g = convex(root_lo, root_hi)
    for J in (0, 1, 5, 16):
        res = ref.search(g, est, g(0.0), delta, n_bisections=J, max_expansions=40)
        assert res.bracketed and res.lower <= root_lo <= est <= root_hi <= res.upper
        # the lower bracket starts as [0, est]; the upper one as the last expansion step
        n_exp = res.n_trials[1] - J
        d = max(est, 1.0)
        first = est if n_exp == 1 else est + d * 2.0 ** (n_exp - 2)
        width = est + d * 2.0 ** (n_exp - 1) - first
        assert res.n_trials[0] >= J and n_exp >= 1
        assert root_lo - res.lower <= est / 2.0**J and res.upper - root_hi <= width / 2.0**J
        # a searched lower end is above 0 and outside: past the J halvings the search goes on to the first trial outside
        assert res.lower > 0.0 and g(res.lower) > delta
        assert res.n_trials[0] == J or (res.lower == res.trace_values[0, res.n_trials[0] - 1] and (res.trace_profile[0, : res.n_trials[0] - 1] <= delta).all())
        assert g(res.upper) > delta
        assert np.array_equal(np.isnan(res.trace_values), np.arange(40 + J)[None, :] >= res.n_trials[:, None])
        # the rule is a function of the g values alone
        again = ref.replay(res.trace_profile, est, g(0.0), delta=delta, n_bisections=J, max_expansions=40)
        for name in ("lower", "upper", "bracketed"):
            assert getattr(again, name) == getattr(res, name)
        assert np.array_equal(again.trace_values, res.trace_values, equal_nan=True) and np.array_equal(again.n_trials, res.n_trials)


def test_search_rule_boundary_and_unbracketed_cases():
    delta = 1.92
    # removing the signature costs no more than the threshold: lower is exactly 0 and nothing is tried for it
    est, g = convex(-2.0, 6.0)
    assert g(0.0) <= delta
    res = ref.search(g, est, g(0.0), delta, n_bisections=8, max_expansions=40)
    assert res.lower == 0.0 and math.copysign(1.0, res.lower) == 1.0 and res.n_trials[0] == 0 and np.isnan(res.trace_values[0]).all()
    assert res.bracketed and res.upper >= 6.0 and res.upper - 6.0 <= 8.0 / 2**8
    # exactly at the threshold counts as inside
    res = ref.search(lambda c: delta, 1.0, delta, delta, n_bisections=3, max_expansions=4)
    assert res.lower == 0.0 and res.upper == np.inf and not res.bracketed and res.n_trials.tolist() == [0, 4]
    assert np.array_equal(res.trace_values[1, :4], [2.0, 3.0, 5.0, 9.0])
    # a flat profile is never bracketed: +inf, no bisection; a small estimate expands from 1.  Its lower end finds nothing outside
    # in the 6 + 3 halvings it is allowed and stays 0.0
    res = ref.search(lambda c: 0.0, 1e-7, 5.0, delta, n_bisections=6, max_expansions=3)
    assert res.upper == np.inf and not res.bracketed and res.n_trials.tolist() == [9, 3]
    assert np.array_equal(res.trace_values[1, :3], [1e-7 + 1.0, 1e-7 + 2.0, 1e-7 + 4.0]) and res.lower == 0.0
    assert np.array_equal(res.trace_values[0, :9], 1e-7 * 0.5 ** np.arange(1, 10))
    # a NaN compares false: inside
    res = ref.search(lambda c: np.nan, 4.0, np.nan, delta, n_bisections=2, max_expansions=2)
    assert res.n_trials.tolist() == [4, 2] and res.upper == np.inf and res.lower == 0.0
    # a root below estimate / 2**J: the halving goes on past J to the first trial outside, and no further
    est, g = convex(0.1, 15.9)
    assert g(0.0) > delta
    for J, extra in ((0, 7), (3, 4), (5, 2), (6, 1), (7, 0), (12, 0)):  # 8 / 2**7 = 0.0625 is the first halving below 0.1
        res = ref.search(g, est, g(0.0), delta, n_bisections=J, max_expansions=40)
        assert res.n_trials[0] == J + extra and 0.0 < res.lower <= 0.1 and g(res.lower) > delta, J
        assert (res.lower == 0.0625) == (J <= 7)
    res = ref.search(g, est, g(0.0), delta, n_bisections=2, max_expansions=3)  # not reached within 2 + 3
    assert res.n_trials[0] == 5 and res.lower == 0.0
    # more than one expansion
    est, g = convex(0.5, 40.0)
    res = ref.search(g, est, g(0.0), delta, n_bisections=4, max_expansions=40)
    assert res.n_trials[1] - 4 == 1  # est + est already lies past the upper root of a symmetric profile
    res = ref.search(lambda c: 0.1 * c, 0.2, 0.0, delta, n_bisections=4, max_expansions=40)
    assert res.n_trials[1] - 4 == 6 and res.lower == 0.0 and 19.2 <= res.upper <= 19.2 + 16.0 / 2**4  # 0.2 + 2^e first exceeds 19.2 at e = 5


def test_the_profile_is_convex_at_converged_solves():
    """f(c) is the minimum over the other exposures of a function jointly convex in h, so it is convex in c; the solves stop at a
    relative change of the objective below tol between tests, so a second difference may miss by a few tol * f."""
    X, W = small_case(N=8, K=4, V=24, seed=5)
    kw = dict(min_iterations=500, max_iterations=20000, conv_test_freq=10, tol=1e-9)
    est = ref.observed(X, W, [1], **kw)[2][:, 1]
    grid = np.linspace(0.0, 2.0, 9)[None, None, :] * np.maximum(est, 1.0)[:, None, None]
    res = ref.profile(X, W, [1], grid, **kw)
    assert res.converged.all()
    f = res.errors[:, 0]
    second = f[:, :-2] - 2.0 * f[:, 1:-1] + f[:, 2:]
    slack = 1e-6 * np.abs(f).max(axis=1, keepdims=True)  # 1000 tol f: the stop rule bounds one test's change, not the distance to the minimum
    print(f"smallest second difference {second.min():.3g}, relative to f {(second / np.abs(f).max(axis=1, keepdims=True)).min():.3g}")
    assert (second >= -slack).all()
    assert (res.profile >= -slack[:, None]).all()  # f1 is the unconstrained minimum


@pytest.fixture(scope="module")
def coverage():
    X, S, E = ref.coverage_samples()
    return X, S, E, ref.intervals(X, S, [0, 3])


def test_coverage_of_an_interior_exposure(coverage):
    """200 Poisson samples of about 2000 mutations from three of four signatures.  The 95 % intervals of the interior signature
    0 must cover its true exposure in at least 0.95 - 3 sqrt(0.95 * 0.05 / 200) = 90.4 % of the samples: 181 of 200."""
    X, S, E, res = coverage
    covered = (res.lower[:, 0] <= E[:, 0]) & (E[:, 0] <= res.upper[:, 0])
    need = math.ceil(200 * (0.95 - 3.0 * math.sqrt(0.95 * 0.05 / 200)))
    print(f"interior signature: {int(covered.sum())} of 200 covered (needed {need}); median width {np.median(res.upper[:, 0] - res.lower[:, 0]):.1f}, "
          f"trials {res.n_trials[:, 0].sum(axis=1).min()}..{res.n_trials[:, 0].sum(axis=1).max()}")
    assert res.tested.all() and res.bracketed[:, 0].all() and need == 181
    assert covered.sum() >= need
    assert (res.lower[:, 0] <= res.estimate[:, 0]).all() and (res.estimate[:, 0] <= res.upper[:, 0]).all()


def test_an_absent_signature_has_lower_end_zero(coverage):
    """Signature 3 is in none of the samples: lower == 0 in at least 90 % of them, and always exactly where the presence
    statistic is at most the threshold."""
    X, S, E, res = coverage
    zero = res.lower[:, 1] == 0.0
    print(f"absent signature: lower == 0 in {int(zero.sum())} of 200; largest upper end {res.upper[:, 1].max():.1f}")
    assert zero.sum() >= 180
    assert np.array_equal(zero, res.statistic[:, 1] <= 1.92)
    assert res.bracketed[:, 1].all() and (res.n_trials[zero, 1, 0] == 0).all()


class FakeLibrary:
    """Stands where ``libsalnmf.so`` would: records the calls that get past the validation and fills nothing."""

    def __init__(self):
        self.calls = []

    def salnmf_profile_likelihood(self, *args):
        self.calls.append(("profile", args))
        return 0

    def salnmf_exposure_intervals(self, *args):
        self.calls.append(("intervals", args))
        return 0


def test_refusals_come_before_the_library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(intervals_mod._lib, "load_with_device", lambda: fake)
    X, W = refit_ref.poisson_catalogue(4, 3, V=10, seed=0)

    def refused(match, *args, **kw):
        for call in (lambda: sal.profile_likelihood(*args, **{"values": [0.0], **kw}), lambda: sal.exposure_intervals(*args, **kw)):
            with pytest.raises(ValueError, match=match):
                call()
        assert not fake.calls

    # what the presence test refuses of the shared arguments
    refused("1 to 96 signatures, got 97", X, np.ones((97, 10)), [0])
    refused("'test' must be a non-empty list of distinct signature indices in \\[0, 3\\)", X, W, [3])
    refused("'test' must be a non-empty list", X, W, [])
    refused("'test' must be a non-empty list", X, W, [1, 1])
    refused("multiple of 'conv_test_freq'", X, W, [0], max_iterations=1005)
    refused("min_iterations <= max_iterations", X, W, [0], min_iterations=700, max_iterations=600)
    refused("'tol'", X, W, [0], tol=float("nan"))
    refused("'candidates' must have shape", X, W, [0], candidates=np.ones((3, 3), dtype=bool))
    refused("finite and non-negative", np.where(np.arange(10) == 2, -1.0, X), W, [0])
    refused("features", X, np.ones((3, 9)), [0])

    # their own
    def one(match, fn, **kw):
        with pytest.raises(ValueError, match=match):
            fn(X, W, [0, 2], **kw)
        assert not fake.calls

    for values in ([], None, "0.5", [-0.1], [float("nan")], [float("inf")], [True], [[0.0, 1.0]], np.zeros((4, 1, 2)), np.zeros((4, 2)), np.zeros((2, 4, 3)),
                   np.zeros(4097), ["a"]):
        one("'values' must hold finite numbers >= 0 in shape \\(M,\\) or \\(4, 2, M\\)", sal.profile_likelihood, values=values)
    for delta in (-0.1, float("nan"), float("inf"), None, "1.92", True):
        one("'max_kl_increase' must be a finite number >= 0", sal.exposure_intervals, max_kl_increase=delta)
    for J in (-1, 65, 2.5, True):
        one("'n_bisections' must be an integer in \\[0, 64\\]", sal.exposure_intervals, n_bisections=J)
    for E in (0, -3, 1001, 1.5):
        one("'max_expansions' must be an integer in \\[1, 1000\\]", sal.exposure_intervals, max_expansions=E)

    # valid calls get as far as the library, with the arguments in the C order; counts need not be integers
    mask = np.array([True, False, True])
    res = sal.profile_likelihood(X + 0.5, W, [2, 0], np.zeros((4, 2, 3)), candidates=mask, max_iterations=600, keep_exposures=True)
    (kind, args), = fake.calls
    assert kind == "profile" and args[2:4] == (4, 10) and args[5] == 3 and args[7] == 2 and args[10:16] == (3, 1, 500, 600, 10, 1e-7)
    for name, shape in (("profile", (4, 2, 3)), ("errors", (4, 2, 3)), ("n_iterations", (4, 2, 3)), ("converged", (4, 2, 3)),
                        ("profile_exposures", (4, 2, 3, 3)), ("exposures", (4, 3)), ("reconstruction_errors", (4,)), ("tested", (4, 2))):
        assert getattr(res, name).shape == shape, name
    # the fake library tested nothing
    assert np.isnan(res.profile).all() and np.isnan(res.profile_exposures).all() and not res.tested.any() and not res.n_iterations.any()
    assert res.test == (2, 0) and np.array_equal(res.candidates, np.broadcast_to(mask, (4, 3))) and res.converged.dtype == bool
    shared = sal.profile_likelihood(X, W, np.array([1]), (0.0, 1.5))
    assert shared.profile.shape == (4, 1, 2) and shared.profile_exposures is None and fake.calls[-1][1][10:12] == (2, 0) and fake.calls[-1][1][8] is None

    res = sal.exposure_intervals(X + 0.25, W, [2, 0], candidates=mask, max_kl_increase=1.35, n_bisections=5, max_expansions=7, keep_trace=True)
    kind, args = fake.calls[-1]
    assert kind == "intervals" and args[2:4] == (4, 10) and args[7] == 2 and args[9:16] == (1.35, 5, 7, 500, 10000, 10, 1e-7)
    for name in ("lower", "upper", "estimate", "statistic", "null_errors", "bracketed", "tested"):
        assert getattr(res, name).shape == (4, 2), name
    assert res.n_trials.shape == (4, 2, 2) and res.n_trials.dtype == np.int32 and res.bracketed.dtype == bool and res.max_kl_increase == 1.35
    assert res.trace_values.shape == (4, 2, 2, 12) and res.trace_profile.shape == (4, 2, 2, 12) and np.isnan(res.trace_values).all()
    assert np.isnan(res.lower).all() and np.isnan(res.upper).all() and not res.n_trials.any() and not res.bracketed.any()
    quiet = sal.exposure_intervals(X, W, [1])
    assert quiet.trace_values is None and quiet.trace_profile is None and fake.calls[-1][1][9:12] == (1.92, 16, 40)
    assert {"profile_likelihood", "ProfileResult", "exposure_intervals", "IntervalResult"} <= set(sal.__all__)
    assert "1.92" in sal.exposure_intervals.__doc__ and "chi2" in sal.exposure_intervals.__doc__
