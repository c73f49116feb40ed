"""The signature-presence test's host side without a device: the replica (tests/_presence_ref.py) against its own contract --
untested pairs, what a pair's draws depend on --, the calibration of the whole procedure on planted data, and every argument
``sal.signature_presence_test`` refuses before it touches a device."""

import numpy as np
import pytest

import _gof_ref as gof_ref
import _presence_ref as ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import presence as presence_mod


def small_case(N=6, K=4, V=10, seed=0):
    X, W = refit_ref.poisson_catalogue(N, K, V=V, seed=seed, mutations=(50, 400))
    return X, W


def test_stream_word_and_the_goodness_of_fit_draw():
    """The replica's draw with the goodness-of-fit word is ``_gof_ref.draw_row``; with the presence word it is another draw."""
    rng = np.random.default_rng(1)
    W = refit_ref.normalize(rng.dirichlet(np.full(7, 0.5), size=3))
    h = rng.uniform(0.5, 50.0, size=3)
    for T in (0, 1, 2, 257, 1000):
        assert np.array_equal(ref.draw_row(h, W, T, 4, 2, 9, gof_ref.GOF_STREAM), gof_ref.draw_row(h, W, T, 4, 2, 9))
    gofd = gof_ref.draw_row(h, W, 1000, 4, 2, 9)
    for s in (0, 1, 95):
        mine = ref.pair_draw(h, W, 1000, 4, s, 2, 9)
        assert mine.sum() == 1000 and not np.array_equal(mine, gofd)
    assert ref.PRESENCE_STREAM == 0x50530000 and ref.PRESENCE_STREAM >> 16 == int.from_bytes(b"PS", "big")
    # 96 stream words, none of them another draw's: the resampler's 0, the split's, the goodness-of-fit draw's
    assert not {ref.PRESENCE_STREAM + s for s in range(96)} & {0, 0x53504C54, gof_ref.GOF_STREAM}


def test_what_a_pairs_draws_depend_on():
    X, W = small_case()
    kw = dict(seed=5, steps=30)
    both = ref.presence(X, W, [0, 2], 4, **kw)
    one = ref.presence(X, W, [2], 4, **kw)
    more = ref.presence(X, W, [2, 3, 1], 8, **kw)
    fewer = ref.presence(X[:3], W, [2], 4, **kw)
    for name in ("statistic", "null_errors", "null_exposures", "n_exceed", "null_mean", "p_value"):
        assert np.array_equal(getattr(one, name)[:, 0], getattr(both, name)[:, 1]), name  # not on S or on what else is tested
    assert np.array_equal(one.null_statistics[:, :, 0], both.null_statistics[:, :, 1])
    assert np.array_equal(one.null_statistics[:, :, 0], more.null_statistics[:4, :, 0])  # not on B
    assert np.array_equal(fewer.null_statistics, one.null_statistics[:, :3])  # not on N
    # the draws themselves: another s, n, seed or b is another draw
    h0, T = one.null_exposures[1, 0], X[1].sum()
    base = ref.pair_draw(h0, W, T, 1, 2, 0, 5)
    assert base.sum() == T and np.array_equal(base, ref.pair_draw(h0, W, T, 1, 2, 0, 5))
    for other in (ref.pair_draw(h0, W, T, 1, 3, 0, 5), ref.pair_draw(h0, W, T, 2, 2, 0, 5), ref.pair_draw(h0, W, T, 1, 2, 0, 6),
                  ref.pair_draw(h0, W, T, 1, 2, 1, 5), gof_ref.draw_row(h0, W, T, 1, 0, 5).astype(np.float64)):
        assert other.sum() == T and not np.array_equal(other, base)
    assert np.array_equal(ref.draws_from(one.null_exposures, W, X.sum(axis=1), [2], one.tested, 2, 5)[0, 1, 0], base)


def test_the_fits_of_a_pair():
    """The alternative is the masked solve on C, the null the one on C without s: exactly 0.0 at s, no better than the alternative
    beyond the iteration's own slack."""
    X, W = small_case(seed=3)
    C = np.ones((6, 4), dtype=bool)
    C[2, 1] = False
    res = ref.presence(X, W, [1, 3], 3, seed=0, candidates=C, steps=200)
    alt = ref.solve(X, W, C, min_iterations=200, max_iterations=200)
    assert np.array_equal(res.exposures, alt.exposures) and np.array_equal(res.reconstruction_errors, alt.reconstruction_errors)
    assert res.exposures[2, 1] == 0.0
    live = res.tested
    assert np.array_equal(live, np.array([[True, True]] * 2 + [[False, True]] + [[True, True]] * 3))
    assert (res.null_exposures[:, 0, 1][live[:, 0]] == 0.0).all() and (res.null_exposures[:, 1, 3] == 0.0).all()
    assert np.array_equal(res.statistic[live], (res.null_errors - res.reconstruction_errors[:, None])[live])
    assert (res.statistic[live] > -1e-6 * res.reconstruction_errors[:, None].repeat(2, axis=1)[live]).all()


def test_untested_pairs():
    X, W = small_case()
    C = np.ones((6, 4), dtype=bool)
    C[0, 2] = False  # s = 2 is no candidate of sample 0
    C[1] = [False, False, True, False]  # C = {2}: nothing to compare with
    C[3] = [True, False, False, False]  # C = {0}: neither tested signature is in it
    res = ref.presence(X, W, [2, 1], 3, seed=1, candidates=C, steps=20)
    want = np.ones((6, 2), dtype=bool)
    want[0, 0] = False
    want[1] = want[3] = False
    assert np.array_equal(res.tested, want)
    for name in ("statistic", "p_value", "null_errors", "null_mean"):
        assert np.array_equal(np.isnan(getattr(res, name)), ~want), name
    assert np.isnan(res.null_statistics[:, ~want]).all() and not np.isnan(res.null_statistics[:, want]).any()
    assert np.isnan(res.exposures[[1, 3]]).all() and not np.isnan(res.exposures[[0, 2, 4, 5]]).any()
    assert not res.n_exceed[~want].any()
    assert np.array_equal(ref.tested_pairs(np.ones((2, 1), dtype=bool), [0]), np.zeros((2, 1), dtype=bool))  # K = 1: all untested
    # the tested pairs of the other samples are what they are without the mask rows
    free = ref.presence(X[[2, 4]], W, [2, 1], 3, seed=1, steps=20)
    assert np.array_equal(free.statistic[0], res.statistic[2])  # sample 0 of `free` is sample 2 here: the fits do not see n
    assert not np.array_equal(free.null_statistics[:, 0], res.null_statistics[:, 2])  # ... the draws do


def test_reduction_rules():
    stat = np.array([[1.0, np.nan], [0.0, -1e-9]])
    null = np.array([[[1.0, 1.0], [0.0, -1e-9]], [[0.5, 2.0], [np.nan, 0.0]], [[2.0, 3.0], [-0.1, -1.0]]])
    n_exceed, mean, p = ref.reduce_null(stat, null)
    assert n_exceed.dtype == np.int32 and n_exceed.tolist() == [[2, 0], [1, 2]]  # ties count, NaNs on either side do not
    assert mean[0, 0] == (0.0 + 1.0 + 0.5 + 2.0) / 3 and np.isnan(mean[1, 0])
    assert p[0, 0] == 3 / 4 and np.isnan(p[0, 1]) and p[1].tolist() == [2 / 4, 3 / 4]


@pytest.fixture(scope="module")
def calibration():
    X, S, s = ref.calibration_samples()
    return X, S, s, ref.presence(X, S, [s], 39, seed=0, steps=300)


def test_calibration_under_the_null(calibration):
    """64 samples of T = 2000 from mixtures of four signatures, tested for a fifth that the generating model does not hold, V = 96,
    B = 39, 300 steps: at most 8 of 64 have p <= 0.05 (Bin(64, 0.05) exceeds 8 with probability below 1 %).  The replica gives 6."""
    X, S, s, res = calibration
    assert X.shape == (72, 96) and S.shape == (5, 96) and s == 4 and np.array_equal(X.sum(axis=1), np.full(72, 2000.0))
    assert res.tested.all() and np.array_equal(res.p_value, (1 + res.n_exceed) / 40)
    null = res.p_value[:64, 0]
    print(f"null samples: {int((null <= 0.05).sum())} of 64 at or below 0.05, mean p {null.mean():.3f}")
    assert (null <= 0.05).sum() <= 8


def test_a_planted_signature_is_found(calibration):
    """8 samples in which the tested signature carries 20 % of the mutations: no null statistic reaches the observed one.  (The
    replica's observed statistics are 146 to 385 times the largest null one.)"""
    _, _, _, res = calibration
    ratio = res.statistic[64:, 0] / res.null_statistics[:, 64:, 0].max(axis=0)
    print(f"planted samples: statistic / largest null statistic {ratio.min():.1f} .. {ratio.max():.1f}")
    assert np.array_equal(res.n_exceed[64:, 0], np.zeros(8, dtype=np.int32))
    assert np.array_equal(res.p_value[64:, 0], np.full(8, 1 / 40))


class FakeLibrary:
    """Stands where ``libsalnmf.so`` would: records the calls that get past the validation and fills nothing."""

    def __init__(self):
        self.calls = []

    def salnmf_signature_presence(self, *args):
        self.calls.append(args)
        return 0


def test_refusals_come_before_the_library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(presence_mod._lib, "load_with_device", lambda: fake)
    X, W = refit_ref.poisson_catalogue(4, 3, V=10, seed=0)

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            sal.signature_presence_test(*args, **kw)
        assert not fake.calls

    refused("1 to 96 signatures, got 97", X, np.ones((97, 10)), [0])
    refused("1 to 96 features, got 97", np.ones((3, 97)), np.ones((2, 97)), [0])
    refused("integer counts: row 1, column 2 holds 0.5", np.where((np.arange(4)[:, None] == 1) & (np.arange(10) == 2), 0.5, X), W, [0])
    big = X.copy()
    big[2, 0] = 2.0**32 - X[2, 1:].sum()
    refused("row totals below 2\\*\\*32: row 2", big, W, [0])
    for test in ([], (), [3], [-1], [0, 0], [1, 2, 1], [0.0], [True], "0", 1, None, [[0]]):
        refused("'test' must be a non-empty list of distinct signature indices in \\[0, 3\\)", X, W, test)
    refused("'n_draws' must be an integer in \\[1, 65536\\]", X, W, [0], n_draws=0)
    for n_draws in (65537, -1, 2.5, True):
        refused("'n_draws'", X, W, [0], n_draws=n_draws)
    refused("multiple of 'conv_test_freq'", X, W, [0], max_iterations=1005)
    refused("multiple of 'conv_test_freq'", X, W, [0], min_iterations=0, max_iterations=10, conv_test_freq=3)
    refused("finite and non-negative", -X, W, [0])
    refused("features", X, np.ones((3, 9)), [0])
    refused("positive sum", X, np.vstack([W[:2], np.zeros((1, 10))]), [0])
    refused("'seed'", X, W, [0], seed=-1)
    refused("'seed'", X, W, [0], seed=2**64)
    refused("min_iterations <= max_iterations", X, W, [0], min_iterations=5, max_iterations=4)
    refused("'conv_test_freq'", X, W, [0], conv_test_freq=0)
    refused("'tol'", X, W, [0], tol=float("nan"))
    refused("'chunk_bytes'", X, W, [0], chunk_bytes=0)
    refused("'candidates' must be a boolean array", X, W, [0], candidates=np.ones(3))
    refused("'candidates' must have shape", X, W, [0], candidates=np.ones((3, 3), dtype=bool))
    refused("Sample 2 has no candidate signature", X, W, [0], candidates=np.arange(4)[:, None] != np.array([2, 2, 2]))

    # a valid call gets as far as the library, with the arguments in the C order
    mask = np.array([True, False, True])
    res = sal.signature_presence_test(X, W, [2, 0], n_draws=5, seed=3, candidates=mask, max_iterations=600, keep_draws=True)
    (args,) = fake.calls
    assert args[2:4] == (4, 10) and args[5] == 3 and args[7] == 2 and args[9:16] == (5, 3, 500, 600, 10, 1e-7, 256 << 20)
    assert res.test == (2, 0) and np.array_equal(res.candidates, np.broadcast_to(mask, (4, 3)))
    for name, shape in (("statistic", (4, 2)), ("p_value", (4, 2)), ("n_exceed", (4, 2)), ("tested", (4, 2)), ("exposures", (4, 3)),
                        ("reconstruction_errors", (4,)), ("null_exposures", (4, 2, 3)), ("null_errors", (4, 2)), ("null_statistics", (5, 4, 2)),
                        ("null_mean", (4, 2)), ("n_iterations", (4, 2, 2)), ("converged", (4, 2, 2)), ("null_n_iterations", (5, 4, 2, 2)),
                        ("draws", (5, 4, 2, 10))):
        assert getattr(res, name).shape == shape, name
    assert res.n_exceed.dtype == np.int32 and res.tested.dtype == bool and res.converged.dtype == bool and res.timings["n_chunks"] == 0
    assert np.isnan(res.p_value).all()  # the fake library tested nothing
    assert sal.signature_presence_test(X, W, np.array([1]), n_draws=1).draws is None and fake.calls[-1][8] is None
    assert {"signature_presence_test", "PresenceResult"} <= set(sal.__all__) and sal.PresenceResult is presence_mod.PresenceResult
