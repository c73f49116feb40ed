"""The per-signature change test's host side without a device: the replica (tests/_sigchange_ref.py) against its own contract --
the stream words, what a problem's results depend on, the tied solve's monotonicity, stationarity and sign, the identities of
equal shares, identical rows and swapped sides, untested problems, the reduction --, the float64 spread the device test's
tolerance is made of, the calibration of the whole procedure, and every argument ``sal.signature_change_test`` refuses before it
touches a device."""

import numpy as np
import pytest

import _assign_masks_ref as masks_ref
import _change_ref as change_ref
import _presence_ref as presence_ref
import _refit_ref as refit_ref
import _sigchange_ref as ref
import salamander_amd as sal
from salamander_amd import sigchange as sigchange_mod

EPS64 = float(np.finfo(np.float64).eps)


def small_case(N=6, K=4, V=10, seed=0):
    Xa, W = refit_ref.poisson_catalogue(N, K, V=V, seed=seed, mutations=(50, 400))
    Xb = np.random.default_rng(100 + seed).poisson(2.0 + 0.5 * Xa[::-1]).astype(np.float64)
    return Xa, Xb, W


dense_case = ref.dense_case


def test_stream_words_and_the_other_draws():
    """The 192 SC words meet none of the five other families', and side and s both change the draw."""
    assert ref.SIGCHANGE_STREAM == 0x53430000 and ref.SIGCHANGE_STREAM >> 16 == int.from_bytes(b"SC", "big")
    mine = {ref.stream_word(s, side) for s in range(96) for side in (0, 1)}
    assert len(mine) == 192 and not mine & ref.OTHER_WORDS and {change_ref.CHANGE_STREAM, 0x50570000, presence_ref.PRESENCE_STREAM} <= ref.OTHER_WORDS
    assert not any(word >> 16 == ref.SIGCHANGE_STREAM >> 16 for word in ref.OTHER_WORDS) and all(word >> 16 == 0x5343 for word in mine)
    rng = np.random.default_rng(1)
    W = refit_ref.normalize(rng.dirichlet(np.full(7, 0.5), size=3))
    h = rng.uniform(0.5, 50.0, size=3)
    seed, n, b, T = 9, 4, 2, 1000
    base = ref.pair_draw(h, W, T, n, 1, 0, b, seed)
    others = [ref.pair_draw(h, W, T, n, 1, 1, b, seed), ref.pair_draw(h, W, T, n, 2, 0, b, seed), ref.pair_draw(h, W, T, n, 0, 1, b, seed),
              change_ref.pair_draw(h, W, T, n, 0, b, seed), presence_ref.pair_draw(h, W, T, n, 1, b, seed),
              ref.pair_draw(h, W, T, n + 1, 1, 0, b, seed), ref.pair_draw(h, W, T, n, 1, 0, b + 1, seed), ref.pair_draw(h, W, T, n, 1, 0, b, seed + 1)]
    assert base.sum() == T and all(o.sum() == T and not np.array_equal(o, base) for o in others)
    assert ref.stream_word(1, 1) != ref.stream_word(2, 0)  # (2 s + side: a signature's side b is not the next one's side a)
    for T in (0, 1, 2, 257):
        assert ref.pair_draw(h, W, T, n, 2, 1, b, seed).sum() == T


def test_what_a_problems_results_depend_on():
    Xa, Xb, W = small_case()
    kw = dict(seed=5, steps=30)
    names = ("statistic", "tied_exposures_a", "tied_exposures_b", "errors")
    base = ref.signature_change(Xa, Xb, W, (0, 2), 4, **kw)
    more = ref.signature_change(Xa, Xb, W, (0, 2), 8, **kw)
    fewer = ref.signature_change(Xa[:3], Xb[:3], W, (0, 2), 4, **kw)
    other = ref.signature_change(Xa, np.vstack([Xb[:3], Xb[3:] + 1.0]), W, (0, 2), 4, **kw)
    one = ref.signature_change(Xa, Xb, W, (2,), 4, **kw)
    assert base.tested.all()
    for name in names:
        assert np.array_equal(getattr(base, name), getattr(more, name)), name  # not on B
        assert np.array_equal(getattr(base, name)[:3], getattr(fewer, name)), name  # not on N
        assert np.array_equal(getattr(base, name)[:3], getattr(other, name)[:3]), name  # not on the other pairs
        assert np.array_equal(getattr(base, name)[:, 1:], getattr(one, name)), name  # not on the other tested signatures
    assert np.array_equal(base.exposures_a, one.exposures_a) and np.array_equal(base.exposures_b, one.exposures_b)
    assert np.array_equal(base.null_statistics, more.null_statistics[:4]) and np.array_equal(base.draws, more.draws[:4])
    assert np.array_equal(base.null_statistics[:, :3], fewer.null_statistics) and np.array_equal(base.null_statistics[:, :3], other.null_statistics[:, :3])
    assert np.array_equal(base.null_statistics[:, :, 1:], one.null_statistics) and np.array_equal(base.draws[:, :, 1:], one.draws)
    assert np.array_equal(base.n_exceed[:3], fewer.n_exceed) and np.array_equal(base.p_value[:, 1:], one.p_value)
    assert not np.array_equal(base.null_statistics[:, 3:], other.null_statistics[:, 3:])
    totals = np.stack([Xa.sum(axis=1), Xb.sum(axis=1)], axis=1)
    assert np.array_equal(base.draws.sum(axis=4), np.broadcast_to(totals[None, :, None, :], (4, 6, 2, 2)))
    moved = ref.signature_change(Xa[[2, 4]], Xb[[2, 4]], W, (0, 2), 4, **kw)  # the fits do not see n, the draws do
    assert np.array_equal(moved.statistic, base.statistic[[2, 4]]) and not np.array_equal(moved.null_statistics, base.null_statistics[:, [2, 4]])
    # the free fits are the masked solves of the contract
    Wn = refit_ref.normalize(W)  # (as the procedure normalises it)
    a, b = presence_ref.solve(Xa, Wn, np.ones((6, 4), dtype=bool), min_iterations=30, max_iterations=30), presence_ref.solve(
        Xb, Wn, np.ones((6, 4), dtype=bool), min_iterations=30, max_iterations=30)
    assert np.array_equal(base.exposures_a, a.exposures) and np.array_equal(base.errors[:, 0, 1], b.reconstruction_errors)
    e = base.errors
    assert np.array_equal(base.statistic, (e[..., 2] - e[..., 0]) + (e[..., 3] - e[..., 1]))


def never_rises(run, Xa, Xb, W):
    """No step of a longdouble history raises the objective by more than the two evaluations' own rounding: 2 V longdouble
    roundings of the rows' scale sum_v |x log(x / p)| + x + p (the sums have V terms each)."""
    scale_a, scale_b = ref.row_scales(Xa, Xb, W, run.exposures_a, run.exposures_b)
    steps = np.diff(run.objectives, axis=0)
    slack = 2 * Xa.shape[1] * float(np.finfo(np.longdouble).eps) * (scale_a + scale_b)
    ratio = float((steps / slack).max())  # (recorded: 0.013, 0.011 and below 0 on the three inputs of the test)
    print(f"largest rise {float(steps.max()):.3g} (slack {float(slack.min()):.3g} or more: at most {ratio:.3g} of it), largest fall {float(-steps.min()):.3g}")
    return bool((steps <= slack).all() and (steps < 0).any())


def test_the_tied_objective_never_rises():
    """In longdouble the tied solve is an EM ascent: f_a0 + f_b0 falls (or stays, within the evaluation's rounding) from every
    step to the next."""
    for (Xa, Xb, W), s in ((small_case(), 0), (small_case(seed=3), 2)):
        C = np.ones((Xa.shape[0], W.shape[0]), dtype=bool)
        C[1, 1] = False
        run = ref.tied_solve(Xa, Xb, W, C, s, min_iterations=120, max_iterations=120, dtype=np.longdouble, history=True)
        assert run.objectives.shape == (121, Xa.shape[0]) and never_rises(run, Xa, Xb, W)
    Xa, Xb, W, C, test = ref.gpu_case(17, 96)
    ns, js, sig = ref.gpu_problems(17, 96)
    run = ref.tied_solve(Xa[ns], Xb[ns], W, C[ns], sig, min_iterations=40, max_iterations=40, dtype=np.longdouble, history=True)
    assert never_rises(run, Xa[ns], Xb[ns], W)


def test_stationarity_at_a_converged_tied_solve():
    """A solve that stops on ``tol`` at a test has moved the objective by less than tol x f over the last conv_test_freq steps.
    Near the optimum a step lowers the objective by about sum_k h_k (u_k - 1)^2 / 2 (the EM decrease to second order), so a factor
    off 1 by d on an entry of share w of the total t costs w t d^2 / 2 per step: |u - 1| <= sqrt(2 tol f / (freq w t)), with a
    factor 2 for the second-order remainder.  The tied entry's factor is c_a u_as + c_b u_bs, of share pi of t_a + t_b."""
    Xa, W = dense_case()
    Xb = np.random.default_rng(3).poisson(0.4 * Xa).astype(np.float64) + 1.0
    C = np.ones((6, 4), dtype=bool)
    tol, freq = 1e-9, 10
    for s in (0, 3):
        run = ref.tied_solve(Xa, Xb, W, C, s, min_iterations=50, max_iterations=5000, conv_test_freq=freq, tol=tol)
        assert run.converged.all()
        xa, xb = np.maximum(Xa, ref.EPSILON), np.maximum(Xb, ref.EPSILON)
        ua, ub = masks_ref.update_factors(xa, W, run.exposures_a), masks_ref.update_factors(xb, W, run.exposures_b)
        ta, tb = run.totals_a, run.totals_b
        F = ta / (ta + tb) * ua[:, s] + tb / (ta + tb) * ub[:, s]
        f = run.errors_a + run.errors_b
        share = (run.exposures_a[:, s] + run.exposures_b[:, s]) / (ta + tb)
        bound = 2 * np.sqrt(2 * tol * f / (freq * share * (ta + tb)))
        print(f"s = {s}: |F - 1| up to {np.abs(F - 1).max():.3g} (bound {bound.min():.3g} .. {bound.max():.3g})")
        assert (np.abs(F - 1) <= bound).all()
        for u, h, t in ((ua, run.exposures_a, ta), (ub, run.exposures_b, tb)):
            free = np.arange(4) != s
            off = h[:, free] > ref.EPSILON  # (an entry at the floor is held there by the clip, whatever its factor)
            limit = 2 * np.sqrt(2 * tol * f[:, None] / (freq * h[:, free]))
            assert off.sum() >= 12 and (np.abs(u[:, free] - 1) <= limit)[off].all()


def test_sign_of_the_statistic():
    """The alternative holds the null: the statistic is not negative beyond rounding -- measured here as the spread of the four
    divergences in two float64 feature orders about the longdouble ones, F_SPREAD of each row's scale -- once both solves have
    converged (the replica at 2000 steps)."""
    Xa, W = dense_case()
    Xb = np.random.default_rng(3).poisson(0.4 * Xa).astype(np.float64) + 1.0
    C = np.ones((6, 4), dtype=bool)
    for s in range(4):
        run = ref.procedure(Xa, Xb, W, C, np.full(6, s), min_iterations=2000, max_iterations=2000)
        scale_a, scale_b = ref.row_scales(Xa, Xb, W, run.tied.exposures_a, run.tied.exposures_b)
        assert (run.statistic >= -4 * ref.F_SPREAD * (scale_a + scale_b)).all() and (run.statistic > 0).any()


@pytest.mark.parametrize("m", [1.0, 2.0, 4.0])
def test_equal_shares_give_a_zero_statistic(m):
    """x_b = m x_a, m a power of two, nothing clipped and nothing at the floor: the free fits are exact multiples (h_b = m h_a,
    f_b = m f_a), both samples have the same update factors at every step, the tied factor of two equal factors is that factor
    (``tied_factor``: the halved sum is exact and the product is zero), so the tied solve is the two free solves and the
    statistic is exactly 0.0.  (With F as the two rounded products c_a u + c_b u it was not, for m > 1: |statistic| up to 2.8e-13,
    since 1 / (1 + m) is no float64 number.)"""
    Xa, W = dense_case()
    C = np.ones((6, 4), dtype=bool)
    for steps in (30, 300):
        for s in (0, 2):
            run = ref.procedure(Xa, m * Xa, W, C, np.full(6, s), min_iterations=steps, max_iterations=steps)
            assert np.array_equal(run.b.exposures, m * run.a.exposures) and np.array_equal(run.b.reconstruction_errors, m * run.a.reconstruction_errors)
            print(f"m = {m}, {steps} steps, s = {s}: |statistic| up to {np.abs(run.statistic).max():.3g}")
            assert (run.statistic == 0.0).all()
            assert np.array_equal(run.tied.exposures_a, run.a.exposures) and np.array_equal(run.tied.exposures_b, run.b.exposures)


def test_identical_rows_and_swapped_sides():
    Xa, Xb, W = small_case(seed=3)
    Xa[2, :4] = 0.0
    C = np.ones((6, 4), dtype=bool)
    C[1, 2] = False
    fit = dict(min_iterations=20, max_iterations=400, conv_test_freq=10, tol=1e-6)
    twin = ref.procedure(Xa, Xa, W, C, np.full(6, 1), **fit)
    assert (twin.statistic == 0.0).all() and 1 < np.unique(twin.tied.n_iterations).size
    for H, f in ((twin.tied.exposures_a, twin.tied.errors_a), (twin.tied.exposures_b, twin.tied.errors_b)):
        assert np.array_equal(H, twin.a.exposures) and np.array_equal(f, twin.a.reconstruction_errors)
    assert np.array_equal(twin.tied.n_iterations, twin.a.dense.n_iterations) and np.array_equal(twin.tied.converged, twin.a.dense.converged)
    one, other = ref.procedure(Xa, Xb, W, C, np.full(6, 1), **fit), ref.procedure(Xb, Xa, W, C, np.full(6, 1), **fit)
    assert np.array_equal(one.statistic, other.statistic) and np.array_equal(one.tied.n_iterations, other.tied.n_iterations)
    assert np.array_equal(one.tied.exposures_a, other.tied.exposures_b) and np.array_equal(one.tied.exposures_b, other.tied.exposures_a)
    assert np.array_equal(one.tied.errors_a, other.tied.errors_b) and np.array_equal(one.tied.errors_b, other.tied.errors_a)
    assert (one.statistic > 0).all()


@pytest.mark.parametrize("K,V", ref.GPU_CASES)
def test_the_device_tests_inputs_and_their_float64_spread(K, V):
    """The inputs of tests/test_gpu_sigchange.py are what its docstring says, and the tied solve in two float64 feature orders
    stays within H_SPREAD and F_SPREAD of the longdouble one on them: the device is held to 16 x these."""
    Xa, Xb, W, C, test = ref.gpu_case(K, V)
    ns, js, sig = ref.gpu_problems(K, V)
    ta, tb = Xa.sum(axis=1), Xb.sum(axis=1)
    assert ta[:5].tolist() == [0, 1, 2, 257, 100000] and tb[1:6].tolist() == [257, 1, 100000, 2, 0] and (ta[:6] != tb[:6]).all()
    assert (W[K - 1] == 0.0).sum() >= 2 and C[9].sum() == 1 and (~C[:, list(test)] & (C.sum(axis=1) > 1)[:, None]).any()
    assert min(test) < 16 and max(test) >= 16 * ((K - 1) // 16) and ns.size % 2 == 1 and ns.size > 8
    dh, df, ld, _ = ref.fixed_spread(K, V)
    print(f"K = {K}, V = {V}: {ns.size} tested problems, float64 spread of the tied exposures {dh:.3g} (H_SPREAD {ref.H_SPREAD:.3g}), of the "
          f"divergences {df:.3g} (F_SPREAD {ref.F_SPREAD:.3g})")
    assert dh <= ref.H_SPREAD and df <= ref.F_SPREAD
    # the tie off the floor, after 40 steps: the bound the device test uses holds on the replica
    rows = np.arange(ns.size)
    run = ref.tied_solve(Xa[ns], Xb[ns], W, C[ns], sig, **ref.GPU_FIXED)
    ha, hb = run.exposures_a[rows, sig], run.exposures_b[rows, sig]
    off = (ha > ref.EPSILON) & (hb > ref.EPSILON)
    share = (ha + hb) / (run.totals_a + run.totals_b)
    assert off.sum() >= ns.size // 2 and (np.abs(ha / run.totals_a - hb / run.totals_b)[off] <= (ref.TIE_ROUNDINGS_PER_STEP * 40 + 4) * EPS64 * share[off]).all()
    if K < 96:  # under the convergence rule one side of a pair stops two tests or more before the other and waits
        a, b = presence_ref.solve(Xa[ns], W, C[ns], **ref.GPU_FIT), presence_ref.solve(Xb[ns], W, C[ns], **ref.GPU_FIT)
        assert (np.abs(a.dense.n_iterations - b.dense.n_iterations) >= 2 * ref.GPU_FIT["conv_test_freq"]).any()


def test_untested_problems():
    Xa, Xb, W = small_case()
    Xa[0] = 0.0  # an empty row a
    Xb[4] = 0.0  # an empty row b
    C = np.ones((6, 4), dtype=bool)
    C[1] = [False, False, True, False]  # one candidate
    C[2, 0] = False  # signature 0 is not a candidate of pair 2
    res = ref.signature_change(Xa, Xb, W, (0, 2), 3, seed=1, candidates=C, steps=20)
    want = np.array([[False, False], [False, False], [False, True], [True, True], [False, False], [True, True]])
    assert np.array_equal(res.tested, want)
    for name in ("statistic", "p_value", "null_mean"):
        assert np.array_equal(np.isnan(getattr(res, name)), ~want), name
    for name in ("tied_exposures_a", "tied_exposures_b", "errors"):
        assert np.array_equal(np.isnan(getattr(res, name)).all(axis=2), ~want) and not np.isnan(getattr(res, name)[want]).any(), name
    assert np.array_equal(np.isnan(res.exposures_a).all(axis=1), ~want.any(axis=1))
    assert np.isnan(res.null_statistics[:, ~want]).all() and not np.isnan(res.null_statistics[:, want]).any()
    assert not res.draws[:, ~want].any() and not res.n_exceed[~want].any()
    assert not ref.tested_problems(Xa, Xb, np.ones((6, 1), dtype=bool), (0,)).any()  # K = 1: all untested


def test_reduction_rules():
    stat = np.array([[1.0, np.nan], [0.0, -1e-9]])
    null = np.array([[[1.0, 1.0], [0.0, -1e-9]], [[0.5, 2.0], [np.nan, 0.0]], [[2.0, 3.0], [-0.1, -1.0]]])
    n_exceed, mean, p = ref.reduce_null(stat, null)
    assert n_exceed.dtype == np.int32 and n_exceed.tolist() == [[2, 0], [1, 2]]  # ties count, NaNs on either side do not
    assert mean[0, 0] == (0.0 + 1.0 + 0.5 + 2.0) / 3 and np.isnan(mean[1, 0])
    assert p[0, 0] == 3 / 4 and np.isnan(p[0, 1]) and p[1].tolist() == [2 / 4, 3 / 4]


@pytest.fixture(scope="module")
def calibration():
    Xa, Xb, S = ref.calibration_pairs()
    return Xa, Xb, S, ref.signature_change(Xa, Xb, S, (ref.CALIBRATION_TEST, 4), 39, seed=0, steps=300)


def test_calibration_under_the_null(calibration):
    """64 pairs with common shares, 2000 and 500 mutations, V = 96, a catalogue of 5, generator seed 20241 (fixed before the first
    run), B = 39, 300 steps, signature 0 tested (common share at least 0.1): at most 8 of 64 have p <= 0.05.  The replica gives 2,
    mean p 0.502 (and 5 of 64 for signature 4, which the condition does not cover)."""
    Xa, Xb, S, res = calibration
    assert ref.CALIBRATION_SEED == 20241 and Xa.shape == Xb.shape == (72, 96) and S.shape == (5, 96)
    assert np.array_equal(Xa.sum(axis=1), np.full(72, 2000.0)) and np.array_equal(Xb.sum(axis=1), np.r_[np.full(64, 500.0), np.full(8, 2000.0)])
    assert res.tested.all() and np.array_equal(res.p_value, (1 + res.n_exceed) / 40)
    null = res.p_value[:64, 0]
    print(f"null pairs: {int((null <= 0.05).sum())} of 64 at or below 0.05, mean p {null.mean():.3f}")
    assert (null <= 0.05).sum() <= 8


def test_a_changed_share_is_found(calibration):
    """8 pairs in which signature 4 has share 0 in a and 1/2 in b, both 2000: no null statistic reaches the observed one.  (The
    replica's observed statistics are 16.7 to 24.6 times the largest null one.)"""
    _, _, _, res = calibration
    ratio = res.statistic[64:, 1] / res.null_statistics[:, 64:, 1].max(axis=0)
    print(f"planted pairs: statistic / largest null statistic {ratio.min():.1f} .. {ratio.max():.1f}")
    assert np.array_equal(res.n_exceed[64:, 1], np.zeros(8, dtype=np.int32))
    assert np.array_equal(res.p_value[64:, 1], np.full(8, 1 / 40))


class FakeLibrary:
    """Stands where ``libsalnmf.so`` would: records the calls that get past the validation and fills nothing."""

    def __init__(self):
        self.calls = []

    def salnmf_signature_change(self, *args):
        self.calls.append(args)
        return 0


def test_refusals_come_before_the_library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(sigchange_mod._lib, "load_with_device", lambda: fake)
    Xa, W = refit_ref.poisson_catalogue(4, 3, V=10, seed=0)
    Xb = Xa[::-1].copy()

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            sal.signature_change_test(*args, **kw)
        assert not fake.calls

    half = np.where((np.arange(4)[:, None] == 1) & (np.arange(10) == 2), 0.5, Xa)
    big = Xa.copy()
    big[2, 0] = 2.0**32 - Xa[2, 1:].sum()
    refused("1 to 96 signatures, got 97", Xa, Xb, np.ones((97, 10)), [0])
    refused("shapes must agree, got \\(4, 10\\) and \\(3, 10\\)", Xa, Xb[:3], W, [0])
    refused("shapes must agree, got \\(4, 10\\) and \\(4, 9\\)", Xa, Xb[:, :9], W, [0])
    refused("'counts_a': .*integer counts: row 1, column 2 holds 0.5", half, Xb, W, [0])
    refused("'counts_b': .*integer counts: row 1, column 2 holds 0.5", Xa, half, W, [0])
    refused("'counts_a': .*row totals below 2\\*\\*32: row 2", big, Xb, W, [0])
    refused("'counts_b': .*row totals below 2\\*\\*32: row 2", Xa, big, W, [0])
    for test in ([], [3], [-1], [0, 0], [0.0], [True], "0", 1):
        refused("'test' must be a non-empty list of distinct signature indices in \\[0, 3\\)", Xa, Xb, W, test)
    refused("'n_draws' must be an integer in \\[1, 65536\\]", Xa, Xb, W, [0], n_draws=0)
    for n_draws in (65537, -1, 2.5, True):
        refused("'n_draws'", Xa, Xb, W, [0], n_draws=n_draws)
    refused("multiple of 'conv_test_freq'", Xa, Xb, W, [0], max_iterations=1005)
    refused("finite and non-negative", -Xa, Xb, W, [0])
    refused("finite and non-negative", Xa, -Xb, W, [0])
    refused("features", Xa, Xb, np.ones((3, 9)), [0])
    refused("positive sum", Xa, Xb, np.vstack([W[:2], np.zeros((1, 10))]), [0])
    refused("'seed'", Xa, Xb, W, [0], seed=-1)
    refused("min_iterations <= max_iterations", Xa, Xb, W, [0], min_iterations=5, max_iterations=4)
    refused("'conv_test_freq'", Xa, Xb, W, [0], conv_test_freq=0)
    refused("'tol'", Xa, Xb, W, [0], tol=float("nan"))
    refused("'chunk_bytes'", Xa, Xb, W, [0], chunk_bytes=0)
    refused("'keep_draws'", Xa, Xb, W, [0], keep_draws=1)
    refused("'candidates' must be a boolean array", Xa, Xb, W, [0], candidates=np.ones(3))
    refused("'candidates' must have shape", Xa, Xb, W, [0], candidates=np.ones((3, 3), dtype=bool))
    refused("Sample 2 has no candidate signature", Xa, Xb, W, [0], candidates=np.arange(4)[:, None] != np.array([2, 2, 2]))

    # a valid call gets as far as the library, with the arguments in the C order
    mask = np.array([True, False, True])
    res = sal.signature_change_test(Xa, Xb, W, [2, 0], n_draws=5, seed=3, candidates=mask, max_iterations=600, keep_draws=True)
    (args,) = fake.calls
    assert args[2:4] == (4, 10) and args[5:7] == (4, 10) and args[8] == 3 and args[10] == 2 and args[12:19] == (5, 3, 500, 600, 10, 1e-7, 256 << 20)
    assert np.array_equal(res.candidates, np.broadcast_to(mask, (4, 3))) and res.test == (2, 0)
    for name, shape in (("statistic", (4, 2)), ("p_value", (4, 2)), ("n_exceed", (4, 2)), ("tested", (4, 2)), ("null_mean", (4, 2)), ("share_a", (4, 2)),
                        ("share_b", (4, 2)), ("share_difference", (4, 2)), ("tied_share", (4, 2)), ("exposures_a", (4, 3)), ("exposures_b", (4, 3)),
                        ("tied_exposures_a", (4, 2, 3)), ("tied_exposures_b", (4, 2, 3)), ("errors", (4, 2, 4)), ("n_iterations", (4, 2, 3)),
                        ("converged", (4, 2, 3)), ("null_statistics", (5, 4, 2)), ("null_n_iterations", (5, 4, 2, 3)), ("draws", (5, 4, 2, 2, 10))):
        assert getattr(res, name).shape == shape, name
    assert res.n_exceed.dtype == np.int32 and res.tested.dtype == bool and res.converged.dtype == bool and res.timings["n_chunks"] == 0
    assert np.isnan(res.p_value).all()  # the fake library tested nothing
    assert sal.signature_change_test(Xa, Xb, W, [1], n_draws=1).draws is None and fake.calls[-1][11] is None
    assert {"signature_change_test", "SignatureChangeResult"} <= set(sal.__all__) and sal.SignatureChangeResult is sigchange_mod.SignatureChangeResult
