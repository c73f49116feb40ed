"""The negative-binomial signature-presence test's host side without a device: the replica (tests/_nb_presence_ref.py) against
its own contract -- the draw words, what a pair's results depend on, untested pairs, the reduction --, its link to the Poisson
test at a large dispersion, the calibration of the whole procedure on gamma-Poisson data, and every argument
``sal.nb_signature_presence_test`` refuses before it touches a device."""

import numpy as np
import pytest

import _nb_presence_ref as ref
import _nb_ref as nb_ref
import _presence_ref as presence_ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import nb as nb_mod
from salamander_amd import presence as presence_mod

# Largest |t_NB(alpha = 1e6) - t_Poisson| / f0_Poisson over the pairs of `small_case` at seeds 0 and 3, 200 steps, measured on the
# CPU: 1.18e-4 (seed 0).  A sanity link between the two models, not an accuracy claim.
LINK_RECORD = 1.2e-4


def small_case(N=6, K=4, V=10, seed=0):
    return refit_ref.poisson_catalogue(N, K, V=V, seed=seed, mutations=(50, 400))


def test_draw_words():
    """((s + 1) << 16) | b: b fills the low half-word, s + 1 the bits above; no word is a draw word of draw_nb_counts /
    nb_goodness_of_fit (b' < 65536: upper half-word 0) and no two (s, b) share one."""
    s, b = np.meshgrid(np.arange(96), np.arange(ref.MAX_DRAWS), indexing="ij")
    words = ((s + 1) << 16) | b
    assert words[3, 7] == ref.draw_word(3, 7) and ref.draw_word(0, 0) == 0x10000 and ref.draw_word(95, 65535) == (96 << 16) | 0xFFFF
    assert words.min() >= ref.MAX_DRAWS  # above every b'
    assert np.unique(words).size == words.size and words.max() < 2**32
    # the draw itself: another word is another draw, and the plain word b is draw_nb_counts' own
    import _nbdraw_ref as nbdraw_ref

    rng = np.random.default_rng(1)
    W = refit_ref.normalize(rng.dirichlet(np.full(7, 0.5), size=3))
    h = rng.uniform(5.0, 50.0, size=3)
    base, failed = ref.pair_draws(h, W, 20.0, 4, 1, [2], 9)
    assert failed == 0
    plain, _ = nbdraw_ref.draw_nb_counts(h[None], W, 20.0, 1, 9, rows=[4], draws=[2], normalize=False)
    same, _ = nbdraw_ref.draw_nb_counts(h[None], W, 20.0, 1, 9, rows=[4], draws=[(2 << 16) | 2], normalize=False)
    assert np.array_equal(same[0], base) and not np.array_equal(plain[0], base)
    for other in (ref.pair_draws(h, W, 20.0, 4, 2, [2], 9), ref.pair_draws(h, W, 20.0, 5, 1, [2], 9), ref.pair_draws(h, W, 20.0, 4, 1, [3], 9),
                  ref.pair_draws(h, W, 20.0, 4, 1, [2], 10)):
        assert not np.array_equal(other[0], base)


def test_what_a_pairs_results_depend_on():
    X, W = small_case()
    alpha = nb_ref.mixed_alpha(6)
    kw = dict(seed=5, steps=30)
    both = ref.presence(X, W, alpha, [0, 2], 4, **kw)
    one = ref.presence(X, W, alpha, [2], 4, **kw)
    more = ref.presence(X, W, alpha, [2, 3, 1], 8, **kw)
    fewer = ref.presence(X[:3], W, alpha[:3], [2], 4, **kw)
    for name in ("statistic", "null_errors", "null_exposures", "n_exceed", "null_mean", "p_value"):
        assert np.array_equal(getattr(one, name)[:, 0], getattr(both, name)[:, 1]), name  # not on S or on what else is tested
    assert np.array_equal(one.null_statistics[:, :, 0], both.null_statistics[:, :, 1])
    assert np.array_equal(one.null_statistics[:, :, 0], more.null_statistics[:4, :, 0])  # not on B
    assert np.array_equal(one.draws[:, :, 0], more.draws[:4, :, 0])
    assert np.array_equal(fewer.null_statistics, one.null_statistics[:, :3])  # not on N
    # the draw is unconditional: the null totals vary
    totals = one.draws[:, :, 0].sum(axis=-1)
    assert (totals != X.sum(axis=1)).any() and np.unique(totals[:, 0]).size > 1
    assert np.array_equal(ref.draws_from(one.null_exposures, W, alpha, [2], one.tested, 4, 5), one.draws)


def test_untested_pairs_and_the_fits():
    X, W = small_case()
    alpha = nb_ref.mixed_alpha(6)
    C = np.ones((6, 4), dtype=bool)
    C[0, 2] = False  # s = 2 is no candidate of sample 0
    C[1] = [False, False, True, False]  # C = {2}: nothing to compare with
    C[3] = [True, False, False, False]  # C = {0}: neither tested signature is in it
    res = ref.presence(X, W, alpha, [2, 1], 3, seed=1, candidates=C, steps=20)
    want = np.ones((6, 2), dtype=bool)
    want[0, 0] = False
    want[1] = want[3] = False
    assert np.array_equal(res.tested, want)
    for name in ("statistic", "p_value", "null_errors", "null_mean"):
        assert np.array_equal(np.isnan(getattr(res, name)), ~want), name
    assert np.isnan(res.null_statistics[:, ~want]).all() and not np.isnan(res.null_statistics[:, want]).any()
    assert np.isnan(res.exposures[[1, 3]]).all() and not np.isnan(res.exposures[[0, 2, 4, 5]]).any()
    assert not res.n_exceed[~want].any() and not res.draws[:, ~want].any()
    assert np.array_equal(ref.tested_pairs(np.ones((2, 1), dtype=bool), [0]), np.zeros((2, 1), dtype=bool))  # K = 1: all untested
    # the fits: the masked negative-binomial solves, exactly 0.0 at s in the null, the statistic one subtraction
    rows = [0, 2, 4, 5]
    alt = ref.solve(X[rows], refit_ref.normalize(W), alpha[rows], C[rows], min_iterations=20, max_iterations=20)
    assert np.array_equal(res.exposures[rows], alt.exposures) and np.array_equal(res.reconstruction_errors[rows], alt.reconstruction_errors)
    assert (res.null_exposures[:, 0, 2][want[:, 0]] == 0.0).all() and (res.null_exposures[:, 1, 1][want[:, 1]] == 0.0).all()
    assert np.array_equal(res.statistic[want], (res.null_errors - res.reconstruction_errors[:, None])[want])


def test_reduction_rules():
    stat = np.array([[1.0, np.nan], [0.0, -1e-9]])
    null = np.array([[[1.0, 1.0], [0.0, -1e-9]], [[0.5, 2.0], [np.nan, 0.0]], [[2.0, 3.0], [-0.1, -1.0]]])
    n_exceed, mean, p = ref.reduce_null(stat, null)
    assert n_exceed.dtype == np.int32 and n_exceed.tolist() == [[2, 0], [1, 2]]  # ties count, NaNs on either side do not
    assert mean[0, 0] == (0.0 + 1.0 + 0.5 + 2.0) / 3 and np.isnan(mean[1, 0])
    assert p[0, 0] == 3 / 4 and np.isnan(p[0, 1]) and p[1].tolist() == [2 / 4, 3 / 4]


def test_a_large_dispersion_is_close_to_the_poisson_test():
    worst = 0.0
    for seed in (0, 3):
        X, W = small_case(seed=seed)
        nb = ref.presence(X, W, 1e6, [0, 2], 1, seed=0, steps=200)
        poisson = presence_ref.presence(X, W, [0, 2], 1, seed=0, steps=200)
        worst = max(worst, float((np.abs(nb.statistic - poisson.statistic) / poisson.null_errors).max()))
    print(f"largest |t_NB(1e6) - t_Poisson| / f0: {worst:.3g} (recorded {LINK_RECORD:.3g})")
    assert worst <= nb_ref.MARGIN * LINK_RECORD


@pytest.fixture(scope="module")
def calibration():
    X, S, s, alpha = ref.calibration_samples()
    nb = ref.presence(X, S, alpha, [s], ref.CALIBRATION_DRAWS, seed=0, steps=300)
    poisson = presence_ref.presence(X[:64], S, [s], ref.CALIBRATION_DRAWS, seed=0, steps=300)
    return X, S, s, alpha, nb, poisson


def test_calibration_under_the_null(calibration):
    """64 gamma-Poisson samples (alpha = 20, mean total 2000, V = 96) generated by four signatures and tested for a fifth, B = 39,
    300 steps: at most 8 of 64 have p <= 0.05.  The replica gives 3 (generator seed 20261; seed 20260 gave 3 too)."""
    X, S, s, alpha, res, _ = calibration
    assert X.shape == (72, 96) and S.shape == (5, 96) and s == 4 and alpha == 20.0 and ref.CALIBRATION_SEED == 20261
    assert res.tested.all() and np.array_equal(res.p_value, (1 + res.n_exceed) / 40)
    null = res.p_value[:64, 0]
    print(f"null samples: {int((null <= 0.05).sum())} of 64 at or below 0.05, mean p {null.mean():.3f}, mean total {X.sum(axis=1).mean():.0f}")
    assert (null <= 0.05).sum() <= ref.CALIBRATION_CAP


def test_a_planted_signature_is_found(calibration):
    """8 samples in which the tested signature carries 20 % of the mean: no null statistic reaches the observed one."""
    res = calibration[4]
    ratio = res.statistic[64:, 0] / res.null_statistics[:, 64:, 0].max(axis=0)
    print(f"planted samples: statistic / largest null statistic {ratio.min():.1f} .. {ratio.max():.1f}")
    assert np.array_equal(res.n_exceed[64:, 0], np.zeros(8, dtype=np.int32))


def test_the_poisson_test_rejects_more_often_on_overdispersed_counts(calibration):
    """On the same 64 null samples the Poisson test (``_presence_ref.presence``) rejects more often than the negative-binomial
    one: the replicas give 5 against 3.  (Generator seed 20260 gave 3 against 3 and was replaced for this condition alone.)"""
    nb, poisson = calibration[4], calibration[5]
    n_nb, n_poisson = int((nb.p_value[:64, 0] <= 0.05).sum()), int((poisson.p_value[:, 0] <= 0.05).sum())
    print(f"rejections at 0.05 of 64: Poisson {n_poisson}, negative binomial {n_nb}")
    assert n_poisson > n_nb


class FakeLibrary:
    """Stands where ``libsalnmf.so`` would: records the calls that get past the validation and fills nothing."""

    def __init__(self):
        self.calls = []

    def salnmf_nb_signature_presence(self, *args):
        self.calls.append(args)
        return 0


def test_refusals_come_before_the_library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(presence_mod._lib, "load_with_device", lambda: fake)
    X, W = refit_ref.poisson_catalogue(4, 3, V=10, seed=0)

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            sal.nb_signature_presence_test(*args, **kw)
        assert not fake.calls

    # the dispersion
    refused("'dispersion' must be a scalar or hold one value per sample \\(4\\)", X, W, np.ones(3), [0])
    refused("'dispersion' must be a scalar or hold one value per sample \\(4\\)", X, W, np.ones((4, 1)), [0])
    refused("'dispersion' must lie in \\(0, 1e\\+06\\]", X, W, 0.0, [0])
    refused("'dispersion' must lie in \\(0, 1e\\+06\\]", X, W, [1.0, 2.0, -1.0, 3.0], [0])
    refused("'dispersion' must lie in \\(0, 1e\\+06\\]", X, W, 2e6, [0])
    refused("'dispersion' must be finite", X, W, float("inf"), [0])
    refused("'dispersion' must be finite", X, W, [1.0, float("nan"), 1.0, 1.0], [0])
    refused("'dispersion' must be a number", X, W, "twenty", [0])
    # section 17's list
    refused("1 to 96 signatures, got 97", X, np.ones((97, 10)), 20.0, [0])
    refused("1 to 96 features, got 97", np.ones((3, 97)), np.ones((2, 97)), 20.0, [0])
    refused("integer counts: row 1, column 2 holds 0.5", np.where((np.arange(4)[:, None] == 1) & (np.arange(10) == 2), 0.5, X), W, 20.0, [0])
    big = X.copy()
    big[2, 0] = 2.0**32 - X[2, 1:].sum()
    refused("row totals below 2\\*\\*32: row 2", big, W, 20.0, [0])
    for test in ([], (), [3], [-1], [0, 0], [1, 2, 1], [0.0], [True], "0", 1, None, [[0]]):
        refused("'test' must be a non-empty list of distinct signature indices in \\[0, 3\\)", X, W, 20.0, test)
    refused("'n_draws' must be an integer in \\[1, 65536\\]", X, W, 20.0, [0], n_draws=0)
    for n_draws in (65537, -1, 2.5, True):
        refused("'n_draws'", X, W, 20.0, [0], n_draws=n_draws)
    refused("multiple of 'conv_test_freq'", X, W, 20.0, [0], max_iterations=1005)
    refused("multiple of 'conv_test_freq'", X, W, 20.0, [0], min_iterations=0, max_iterations=10, conv_test_freq=3)
    refused("finite and non-negative", -X, W, 20.0, [0])
    refused("features", X, np.ones((3, 9)), 20.0, [0])
    refused("positive sum", X, np.vstack([W[:2], np.zeros((1, 10))]), 20.0, [0])
    refused("'seed'", X, W, 20.0, [0], seed=-1)
    refused("'seed'", X, W, 20.0, [0], seed=2**64)
    refused("min_iterations <= max_iterations", X, W, 20.0, [0], min_iterations=5, max_iterations=4)
    refused("'conv_test_freq'", X, W, 20.0, [0], conv_test_freq=0)
    refused("'tol'", X, W, 20.0, [0], tol=float("nan"))
    refused("'chunk_bytes'", X, W, 20.0, [0], chunk_bytes=0)
    refused("'candidates' must be a boolean array", X, W, 20.0, [0], candidates=np.ones(3))
    refused("'candidates' must have shape", X, W, 20.0, [0], candidates=np.ones((3, 3), dtype=bool))
    refused("Sample 2 has no candidate signature", X, W, 20.0, [0], candidates=np.arange(4)[:, None] != np.array([2, 2, 2]))

    # a valid call gets as far as the library, with the arguments in the C order: the dispersions after K, the failure count last
    mask = np.array([True, False, True])
    res = sal.nb_signature_presence_test(X, W, 20.0, [2, 0], n_draws=5, seed=3, candidates=mask, max_iterations=600, keep_draws=True)
    (args,) = fake.calls
    assert len(args) == 32 and args[2:4] == (4, 10) and args[5] == 3 and args[8] == 2 and args[10:17] == (5, 3, 500, 600, 10, 1e-7, 256 << 20)
    assert np.array_equal(np.ctypeslib.as_array(args[6], shape=(4,)), np.full(4, 20.0))
    assert isinstance(res, sal.NBPresenceResult) and isinstance(res, sal.PresenceResult)
    assert res.test == (2, 0) and np.array_equal(res.candidates, np.broadcast_to(mask, (4, 3))) and np.array_equal(res.dispersion, np.full(4, 20.0))
    for name, shape in (("statistic", (4, 2)), ("p_value", (4, 2)), ("n_exceed", (4, 2)), ("tested", (4, 2)), ("exposures", (4, 3)),
                        ("reconstruction_errors", (4,)), ("null_exposures", (4, 2, 3)), ("null_errors", (4, 2)), ("null_statistics", (5, 4, 2)),
                        ("null_mean", (4, 2)), ("n_iterations", (4, 2, 2)), ("converged", (4, 2, 2)), ("null_n_iterations", (5, 4, 2, 2)),
                        ("draws", (5, 4, 2, 10)), ("dispersion", (4,)), ("log_likelihood", (4,)), ("null_log_likelihood", (4, 2))):
        assert getattr(res, name).shape == shape, name
    assert np.isnan(res.p_value).all()  # the fake library tested nothing
    assert sal.nb_signature_presence_test(X, W, np.full(4, 0.5), np.array([1]), n_draws=1).draws is None and fake.calls[-1][9] is None
    assert {"nb_signature_presence_test", "NBPresenceResult"} <= set(sal.__all__) and sal.NBPresenceResult is nb_mod.NBPresenceResult
