"""The exposure-change test's host side without a device: the replica (tests/_change_ref.py) against its own contract -- the
stream word, what a pair's results depend on, the identity with the G statistic of the 2 x V table, untested pairs, the
reduction --, the float64 spread the device test's tolerance is made of, the calibration of the whole procedure, and every
argument ``sal.exposure_change_test`` refuses before it touches a device."""

import numpy as np
import pytest

import _change_ref as ref
import _gof_ref as gof_ref
import _presence_ref as presence_ref
import _refit_ref as refit_ref
import _resample_ref as resample_ref
import salamander_amd as sal
from salamander_amd import change as change_mod


def small_case(N=6, K=4, V=10, seed=0):
    Xa, W = refit_ref.poisson_catalogue(N, K, V=V, seed=seed, mutations=(50, 400))
    Xb = np.random.default_rng(100 + seed).poisson(2.0 + 0.5 * Xa[::-1]).astype(np.float64)
    return Xa, Xb, W


def test_stream_word_and_the_other_draws():
    """The draw with the CH words is none of the other four draws at the same (seed, n, b), and side 0 is not side 1."""
    assert ref.CHANGE_STREAM == 0x43480000 and ref.CHANGE_STREAM >> 16 == int.from_bytes(b"CH", "big")
    # the words of the two sides against every family: the resampler's 0, the split's, the goodness-of-fit draw's, and the 96
    # words each of the presence test and of its power analysis
    taken = {0, 0x53504C54, gof_ref.GOF_STREAM} | {presence_ref.PRESENCE_STREAM + s for s in range(96)} | {0x50570000 + s for s in range(96)}
    assert set(ref.OTHER_STREAMS.values()) <= taken and not {ref.CHANGE_STREAM, ref.CHANGE_STREAM + 1} & taken
    assert not any(word >> 16 == ref.CHANGE_STREAM >> 16 for word in taken)
    rng = np.random.default_rng(1)
    W = refit_ref.normalize(rng.dirichlet(np.full(7, 0.5), size=3))
    h = rng.uniform(0.5, 50.0, size=3)
    seed, n, b, T = 9, 4, 2, 1000
    side0, side1 = ref.pair_draw(h, W, T, n, 0, b, seed), ref.pair_draw(h, W, T, n, 1, b, seed)
    assert side0.sum() == T and side1.sum() == T and not np.array_equal(side0, side1)
    others = {"gof": gof_ref.draw_row(h, W, T, n, b, seed), "presence": presence_ref.pair_draw(h, W, T, n, 0, b, seed),
              "presence 1": presence_ref.pair_draw(h, W, T, n, 1, b, seed)}
    # the resampler and the split draw from integer counts with a 32-bit table, not from a spectrum: at the same counter words
    # their Philox blocks differ from this stream's, which is what keeps the streams apart
    q = np.arange(4, dtype=np.uint64)
    mine = resample_ref.philox4x32_10(q, np.full_like(q, ref.CHANGE_STREAM), np.full_like(q, n), np.full_like(q, b), seed, 0)
    for word in (0, 0x53504C54):
        theirs = resample_ref.philox4x32_10(q, np.full_like(q, word), np.full_like(q, n), np.full_like(q, b), seed, 0)
        assert not any(np.array_equal(x, y) for x, y in zip(mine, theirs))
    for name, other in others.items():
        assert other.sum() == T and not np.array_equal(other, side0) and not np.array_equal(other, side1), name
    for T in (0, 1, 2, 257):
        assert ref.pair_draw(h, W, T, n, 1, b, seed).sum() == T
    assert np.array_equal(presence_ref.draw_row(h, W, 257, n, b, seed, ref.CHANGE_STREAM + 1), ref.pair_draw(h, W, 257, n, 1, b, seed))


def test_what_a_pairs_results_depend_on():
    Xa, Xb, W = small_case()
    kw = dict(seed=5, steps=30)
    base = ref.change(Xa, Xb, W, 4, **kw)
    more = ref.change(Xa, Xb, W, 8, **kw)
    fewer = ref.change(Xa[:3], Xb[:3], W, 4, **kw)
    other = ref.change(Xa, np.vstack([Xb[:3], Xb[3:] + 1.0]), W, 4, **kw)
    assert base.tested.all()
    for name in ("statistic", "exposures_a", "exposures_b", "pooled_exposures", "errors", "null_errors"):
        assert np.array_equal(getattr(base, name), getattr(more, name)), name  # not on B
        assert np.array_equal(getattr(base, name)[:3], getattr(fewer, name)), name  # not on N
        assert np.array_equal(getattr(base, name)[:3], getattr(other, name)[:3]), name  # not on the other pairs
    assert np.array_equal(base.null_statistics, more.null_statistics[:4]) and np.array_equal(base.draws, more.draws[:4])
    assert np.array_equal(base.null_statistics[:, :3], fewer.null_statistics) and np.array_equal(base.null_statistics[:, :3], other.null_statistics[:, :3])
    assert np.array_equal(base.n_exceed[:3], fewer.n_exceed) and np.array_equal(base.p_value[:3], fewer.p_value)
    assert not np.array_equal(base.null_statistics[:, 3:], other.null_statistics[:, 3:])
    # the draws themselves: the totals are the two samples' own; another n, seed, b or side is another draw
    assert np.array_equal(base.draws.sum(axis=3), np.broadcast_to(np.stack([Xa.sum(axis=1), Xb.sum(axis=1)], axis=1), (4, 6, 2)))
    h0, T = base.pooled_exposures[1], Xa[1].sum()
    mine = ref.pair_draw(h0, W, T, 1, 0, 0, 5)
    assert np.array_equal(mine, base.draws[0, 1, 0])
    for changed in (ref.pair_draw(h0, W, T, 2, 0, 0, 5), ref.pair_draw(h0, W, T, 1, 0, 0, 6), ref.pair_draw(h0, W, T, 1, 0, 1, 5),
                    ref.pair_draw(h0, W, T, 1, 1, 0, 5)):
        assert changed.sum() == T and not np.array_equal(changed, mine)
    # the fits do not see n, the draws do
    moved = ref.change(Xa[[2, 4]], Xb[[2, 4]], W, 4, **kw)
    assert np.array_equal(moved.statistic, base.statistic[[2, 4]]) and not np.array_equal(moved.null_statistics, base.null_statistics[:, [2, 4]])


def test_the_three_fits_and_the_statistic():
    """The fits are the masked solves of the contract, the pooled one on the sum of the CLIPPED rows; the statistic is composed
    in the stated order and is not negative beyond the iteration's slack (the alternative holds the null)."""
    Xa, Xb, W = small_case(seed=3)
    Xa[2, :4] = 0.0
    C = np.ones((6, 4), dtype=bool)
    C[1, 2] = False
    res = ref.change(Xa, Xb, W, 2, seed=0, candidates=C, steps=200)
    kw = dict(min_iterations=200, max_iterations=200)
    a, b = presence_ref.solve(Xa, W, C, **kw), presence_ref.solve(Xb, W, C, **kw)
    pooled = presence_ref.solve(np.maximum(Xa, ref.EPSILON) + np.maximum(Xb, ref.EPSILON), W, C, **kw)
    assert np.array_equal(res.exposures_a, a.exposures) and np.array_equal(res.exposures_b, b.exposures)
    assert np.array_equal(res.pooled_exposures, pooled.exposures) and res.pooled_exposures[1, 2] == 0.0
    assert np.array_equal(res.errors, np.stack([a.reconstruction_errors, b.reconstruction_errors, pooled.reconstruction_errors], axis=1))
    assert np.array_equal(res.statistic, (res.null_errors[:, 0] - res.errors[:, 0]) + (res.null_errors[:, 1] - res.errors[:, 1]))
    assert (res.statistic > -1e-6 * res.errors.sum(axis=1)).all()
    # with the same shares on both sides the null divergences are the samples' own fits: the statistic of a multiple of the row is
    # zero within the same slack (the clipped zeros do not scale, and the three 200-step solves end at slightly different points)
    same = ref.change(Xa, 3.0 * Xa, W, 1, steps=200)
    assert (np.abs(same.statistic) < 1e-6 * same.errors.sum(axis=1)).all()


def test_the_identity_with_the_table_statistic():
    """g_a + g_b - f_p = D, the G statistic of the 2 x V table, whatever the pooled fit (module docstring of the replica): on the
    replica it holds to IDENTITY_BOUND = 16 x the deviation measured here against a longdouble D, relative to the two null
    divergences' scales.  So the statistic is D - (f_a + f_b - f_p): the raw-spectrum statistic less what the catalogue explains."""
    worst = 0.0
    for Xa, Xb, W, steps in ref.identity_cases():
        kw = dict(min_iterations=steps, max_iterations=steps)
        run = ref.procedure(Xa, Xb, W, np.ones((Xa.shape[0], W.shape[0]), dtype=bool), **kw)
        D, _ = ref.table_statistic(Xa, Xb)
        _, _, scale_a, scale_b = ref.null_divergences(Xa, Xb, W, run.pooled.exposures)
        lhs = run.ga + run.gb - run.pooled.reconstruction_errors
        worst = max(worst, float((np.abs(lhs - D) / (scale_a + scale_b)).max()))
        assert (D > 1.0).all()  # (the identity is not tested on zeros)
    print(f"identity: largest |(g_a + g_b - f_p) - D| / scale {worst:.3g} (bound {ref.IDENTITY_BOUND:.3g})")
    assert worst <= ref.IDENTITY_BOUND


@pytest.mark.parametrize("K,V", ref.GPU_CASES)
def test_the_device_tests_inputs_and_their_float64_spread(K, V):
    """The inputs of tests/test_gpu_change.py are what its docstring says, and g_a, g_b in two float64 feature orders stay
    within G_SPREAD of the longdouble evaluation on them: the device is held to 16 x G_SPREAD."""
    Xa, Xb, W, C = ref.gpu_case(K, V)
    N = ref.GPU_N
    assert Xa.shape == Xb.shape == (N, V) and W.shape == (K, V) and C.shape == (N, K)
    assert np.array_equal(Xa, np.floor(Xa)) and np.array_equal(Xb, np.floor(Xb))
    ta, tb = Xa.sum(axis=1), Xb.sum(axis=1)
    assert ta[:5].tolist() == [0, 1, 2, 257, 100000] and tb[1:6].tolist() == [257, 1, 100000, 2, 0] and (ta[:6] != tb[:6]).all()
    assert (W[K - 1] == 0.0).sum() >= 2 and C[9].sum() == 1
    tested = ref.tested_pairs(Xa, Xb, C)
    if K == 1:
        assert not tested.any()
    else:
        assert not tested[[0, 5, 9]].any() and tested[[1, 2, 3, 4]].all() and tested.sum() >= 30
    spread = ref.g_spread(K, V)
    print(f"K = {K}, V = {V}: {int(tested.sum())} tested pairs, float64 spread of g_a, g_b {spread:.3g} (G_SPREAD {ref.G_SPREAD:.3g})")
    assert spread <= ref.G_SPREAD


def test_untested_pairs():
    Xa, Xb, W = small_case()
    Xa[0] = 0.0  # an empty row a
    Xb[4] = 0.0  # an empty row b
    C = np.ones((6, 4), dtype=bool)
    C[1] = [False, False, True, False]  # one candidate: the shares are fixed, nothing to test
    res = ref.change(Xa, Xb, W, 3, seed=1, candidates=C, steps=20)
    want = np.array([False, False, True, True, False, True])
    assert np.array_equal(res.tested, want)
    for name in ("statistic", "p_value", "null_mean"):
        assert np.array_equal(np.isnan(getattr(res, name)), ~want), name
    for name in ("exposures_a", "exposures_b", "pooled_exposures", "errors", "null_errors"):
        assert np.array_equal(np.isnan(getattr(res, name)).all(axis=1), ~want) and not np.isnan(getattr(res, name)[want]).any(), name
    assert np.isnan(res.null_statistics[:, ~want]).all() and not np.isnan(res.null_statistics[:, want]).any()
    assert not res.draws[:, ~want].any() and not res.n_exceed[~want].any()
    assert not ref.tested_pairs(Xa, Xb, np.ones((6, 1), dtype=bool)).any()  # K = 1: all untested
    # the tested pairs are what they are without the others
    free = ref.change(Xa[[2, 3]], Xb[[2, 3]], W, 3, seed=1, steps=20)
    assert np.array_equal(free.statistic, res.statistic[[2, 3]])


def test_reduction_rules():
    stat = np.array([1.0, np.nan, 0.0, -1e-9])
    null = np.array([[1.0, 1.0, 0.0, -1e-9], [0.5, 2.0, np.nan, 0.0], [2.0, 3.0, -0.1, -1.0]])
    n_exceed, mean, p = ref.reduce_null(stat, null)
    assert n_exceed.dtype == np.int32 and n_exceed.tolist() == [2, 0, 1, 2]  # ties count, NaNs on either side do not
    assert mean[0] == (0.0 + 1.0 + 0.5 + 2.0) / 3 and np.isnan(mean[2])
    assert p[0] == 3 / 4 and np.isnan(p[1]) and p[2:].tolist() == [2 / 4, 3 / 4]


@pytest.fixture(scope="module")
def calibration():
    Xa, Xb, S = ref.calibration_pairs()
    return Xa, Xb, S, ref.change(Xa, Xb, S, 39, seed=0, steps=300)


def test_calibration_under_the_null(calibration):
    """64 pairs with common shares, 2000 and 500 mutations, V = 96, a catalogue of 5, generator seed 20240, B = 39, 300 steps: at
    most 8 of 64 have p <= 0.05 (Bin(64, 0.05) exceeds 8 with probability below 1 %).  The replica gives 4."""
    Xa, Xb, S, res = calibration
    assert ref.CALIBRATION_SEED == 20240 and Xa.shape == Xb.shape == (72, 96) and S.shape == (5, 96)
    assert np.array_equal(Xa.sum(axis=1), np.full(72, 2000.0)) and np.array_equal(Xb.sum(axis=1), np.r_[np.full(64, 500.0), np.full(8, 2000.0)])
    assert res.tested.all() and np.array_equal(res.p_value, (1 + res.n_exceed) / 40)
    null = res.p_value[:64]
    print(f"null pairs: {int((null <= 0.05).sum())} of 64 at or below 0.05, mean p {null.mean():.3f}")
    assert (null <= 0.05).sum() <= 8


def test_changed_shares_are_found(calibration):
    """8 pairs in which b has half its mutations from a signature that a does not show: no null statistic reaches the observed
    one.  (The replica's observed statistics are 45 to 106 times the largest null one.)"""
    _, _, _, res = calibration
    ratio = res.statistic[64:] / res.null_statistics[:, 64:].max(axis=0)
    print(f"planted pairs: statistic / largest null statistic {ratio.min():.1f} .. {ratio.max():.1f}")
    assert np.array_equal(res.n_exceed[64:], np.zeros(8, dtype=np.int32))
    assert np.array_equal(res.p_value[64:], np.full(8, 1 / 40))


class FakeLibrary:
    """Stands where ``libsalnmf.so`` would: records the calls that get past the validation and fills nothing."""

    def __init__(self):
        self.calls = []

    def salnmf_exposure_change(self, *args):
        self.calls.append(args)
        return 0


def test_refusals_come_before_the_library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(change_mod._lib, "load_with_device", lambda: fake)
    Xa, W = refit_ref.poisson_catalogue(4, 3, V=10, seed=0)
    Xb = Xa[::-1].copy()

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            sal.exposure_change_test(*args, **kw)
        assert not fake.calls

    half = np.where((np.arange(4)[:, None] == 1) & (np.arange(10) == 2), 0.5, Xa)
    big = Xa.copy()
    big[2, 0] = 2.0**32 - Xa[2, 1:].sum()
    refused("1 to 96 signatures, got 97", Xa, Xb, np.ones((97, 10)))
    refused("1 to 96 features, got 97", np.ones((3, 97)), np.ones((3, 97)), np.ones((2, 97)))
    refused("shapes must agree, got \\(4, 10\\) and \\(3, 10\\)", Xa, Xb[:3], W)
    refused("shapes must agree, got \\(4, 10\\) and \\(4, 9\\)", Xa, Xb[:, :9], W)
    refused("shapes must agree", Xa, Xb[0], W)
    refused("'counts_a': .*integer counts: row 1, column 2 holds 0.5", half, Xb, W)
    refused("'counts_b': .*integer counts: row 1, column 2 holds 0.5", Xa, half, W)
    refused("'counts_a': .*row totals below 2\\*\\*32: row 2", big, Xb, W)
    refused("'counts_b': .*row totals below 2\\*\\*32: row 2", Xa, big, W)
    refused("'n_draws' must be an integer in \\[1, 65536\\]", Xa, Xb, W, n_draws=0)
    for n_draws in (65537, -1, 2.5, True):
        refused("'n_draws'", Xa, Xb, W, n_draws=n_draws)
    refused("multiple of 'conv_test_freq'", Xa, Xb, W, max_iterations=1005)
    refused("multiple of 'conv_test_freq'", Xa, Xb, W, min_iterations=0, max_iterations=10, conv_test_freq=3)
    refused("finite and non-negative", -Xa, Xb, W)
    refused("finite and non-negative", Xa, -Xb, W)
    refused("features", Xa, Xb, np.ones((3, 9)))
    refused("positive sum", Xa, Xb, np.vstack([W[:2], np.zeros((1, 10))]))
    refused("'seed'", Xa, Xb, W, seed=-1)
    refused("'seed'", Xa, Xb, W, seed=2**64)
    refused("min_iterations <= max_iterations", Xa, Xb, W, min_iterations=5, max_iterations=4)
    refused("'conv_test_freq'", Xa, Xb, W, conv_test_freq=0)
    refused("'tol'", Xa, Xb, W, tol=float("nan"))
    refused("'chunk_bytes'", Xa, Xb, W, chunk_bytes=0)
    refused("'keep_draws'", Xa, Xb, W, keep_draws=1)
    refused("'candidates' must be a boolean array", Xa, Xb, W, candidates=np.ones(3))
    refused("'candidates' must have shape", Xa, Xb, W, candidates=np.ones((3, 3), dtype=bool))
    refused("Sample 2 has no candidate signature", Xa, Xb, W, candidates=np.arange(4)[:, None] != np.array([2, 2, 2]))

    # a valid call gets as far as the library, with the arguments in the C order
    mask = np.array([True, False, True])
    res = sal.exposure_change_test(Xa, Xb, W, n_draws=5, seed=3, candidates=mask, max_iterations=600, keep_draws=True)
    (args,) = fake.calls
    assert args[2:4] == (4, 10) and args[5:7] == (4, 10) and args[8] == 3 and args[10:17] == (5, 3, 500, 600, 10, 1e-7, 256 << 20)
    assert np.array_equal(res.candidates, np.broadcast_to(mask, (4, 3)))
    for name, shape in (("statistic", (4,)), ("p_value", (4,)), ("n_exceed", (4,)), ("tested", (4,)), ("null_mean", (4,)), ("exposures_a", (4, 3)),
                        ("exposures_b", (4, 3)), ("pooled_exposures", (4, 3)), ("errors", (4, 3)), ("null_errors", (4, 2)), ("n_iterations", (4, 3)),
                        ("converged", (4, 3)), ("shares_a", (4, 3)), ("shares_b", (4, 3)), ("share_difference", (4, 3)), ("null_statistics", (5, 4)),
                        ("null_n_iterations", (5, 4, 3)), ("draws", (5, 4, 2, 10))):
        assert getattr(res, name).shape == shape, name
    assert res.n_exceed.dtype == np.int32 and res.tested.dtype == bool and res.converged.dtype == bool and res.timings["n_chunks"] == 0
    assert np.isnan(res.p_value).all()  # the fake library tested nothing
    assert sal.exposure_change_test(Xa, Xb, W, n_draws=1).draws is None and fake.calls[-1][9] is None
    assert {"exposure_change_test", "ChangeResult"} <= set(sal.__all__) and sal.ChangeResult is change_mod.ChangeResult
    # the shares are rows of exposures over their sums, and b - a
    H = np.array([[1.0, 3.0], [np.nan, np.nan]])
    assert np.array_equal(change_mod.shares(H), np.array([[0.25, 0.75], [np.nan, np.nan]]), equal_nan=True)
