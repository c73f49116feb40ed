"""The goodness-of-fit test's host side without a device: the replica of the model draw (tests/_gof_ref.py) against its own
contract, the draw's distribution, the calibration of the whole procedure on planted data, and every argument
``sal.goodness_of_fit`` and ``sal.draw_model_counts`` refuse before they touch a device."""

import math

import numpy as np
import pytest

import _gof_ref as ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import gof as gof_mod


def small_model(K=3, V=7, seed=0):
    rng = np.random.default_rng(seed)
    W = refit_ref.normalize(rng.dirichlet(np.full(V, 0.5), size=K))
    h = rng.uniform(0.5, 50.0, size=K)
    return h, W


def test_high_half_of_the_product_against_python_integers():
    rng = np.random.default_rng(1)
    ulo = rng.integers(0, 2**32, size=2000, dtype=np.uint64)
    uhi = rng.integers(0, 2**32, size=2000, dtype=np.uint64)
    ulo[:4], uhi[:4] = (0, 0xFFFFFFFF, 0, 0xFFFFFFFF), (0, 0xFFFFFFFF, 0xFFFFFFFF, 0)
    for M in (1, 2**40, 96 * 2**40, 2**47 - 1, 0x1234_5678_9ABC):
        got = ref.mulhi(ulo, uhi, M)
        want = [((int(h) << 32 | int(l)) * M) >> 64 for l, h in zip(ulo, uhi)]
        assert [int(t) for t in got] == want, M


def test_weights_follow_the_contract():
    h, W = small_model()
    W[1, 2] = 0.0
    W[:, 5] = 0.0
    W = refit_ref.normalize(W)
    P, S = ref.spectrum(h, W)
    want = h[0] * W[0]
    want = want + h[1] * W[1]
    want = want + h[2] * W[2]
    assert np.array_equal(P, want) and S == sum((float(p) for p in P), 0.0)
    m, cum = ref.weights(h, W)
    assert m.dtype == np.uint64 and m[5] == 0 and int(cum[-1]) == sum(int(x) for x in m)
    assert [int(x) for x in m] == [int(math.floor(float(p) / S * 2.0**40)) for p in P]
    assert 2**40 - 7 <= int(cum[-1]) <= 2**40 + 7  # each weight loses less than one unit, the ratios sum to one within rounding
    assert ref.weights(np.zeros(3), W) is None and ref.weights(np.array([1.0, np.inf, 1.0]), W) is None


def test_contract_properties_of_the_draws():
    rng = np.random.default_rng(2)
    K, V, N = 3, 7, 9
    W = rng.dirichlet(np.full(V, 0.5), size=K)
    W[:, 4] = 0.0  # a cell of weight 0
    W = refit_ref.normalize(W)
    H = rng.uniform(0.0, 20.0, size=(N, K))
    H[3] = 0.0  # a model without mass
    totals = np.array([0, 1, 2, 255, 256, 257, 1000, 31, 31])
    H[8] = H[7]  # two rows with the same model and total
    d4 = ref.draw_model_counts(H, W, totals, 4, seed=5)
    d8 = ref.draw_model_counts(H, W, totals, 8, seed=5)
    assert np.array_equal(d4, d8[:4])  # draw b does not depend on B
    live = np.arange(N) != 3
    assert np.array_equal(d8[:, live].sum(axis=2), np.broadcast_to(totals[live], (8, live.sum())))  # row totals are T
    assert not d8[:, 3].any() and not d8[:, 0].any()  # no mass, T = 0
    assert not d8[:, :, 4].any()  # m_v = 0 stays 0
    assert (d8 == np.floor(d8)).all() and (d8 >= 0).all()
    other = ref.draw_model_counts(H, W, totals, 8, seed=6)
    assert not np.array_equal(other[:, 6], d8[:, 6])  # another seed
    assert not np.array_equal(d8[:, 7], d8[:, 8])  # another n, same model
    assert not np.array_equal(d8[0, 6], d8[1, 6])  # another b
    # the stream word: not the resampler's blocks (second counter word 0), not the split's
    from _resample_ref import philox4x32_10

    q = np.arange(4, dtype=np.uint64)
    mine = philox4x32_10(q, np.full_like(q, ref.GOF_STREAM), np.full_like(q, 6), np.full_like(q, 0), 5, 0)
    for stream in (0, 0x53504C54):
        theirs = philox4x32_10(q, np.full_like(q, stream), np.full_like(q, 6), np.full_like(q, 0), 5, 0)
        assert not any(np.array_equal(a, b) for a, b in zip(mine, theirs))


def chi2_6_upper_tail(x):
    """P(chi-square with 6 degrees of freedom > x), in closed form for an even number of degrees."""
    return math.exp(-x / 2) * (1 + x / 2 + x * x / 8)


def test_distribution_of_the_draws():
    """One row, K = 3, V = 7, T = 20 000, B = 50: the pooled chi-square of the bin counts against T B P_v / S lies below the
    1 - 1e-6 quantile of chi-square with 6 degrees of freedom (38.26).  The replica gives 4.32."""
    h, W = small_model(seed=3)
    T, B = 20000, 50
    P, S = ref.spectrum(h, W)
    drawn = ref.draw_model_counts(h[None, :], W, [T], B, seed=0)
    assert drawn.shape == (B, 1, 7)
    observed = drawn[:, 0].sum(axis=0)
    expected = T * B * P / S
    stat = float(((observed - expected) ** 2 / expected).sum())
    lo, hi = 0.0, 200.0
    for _ in range(200):  # the quantile by bisection of the closed form
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi2_6_upper_tail(mid) > 1e-6 else (lo, mid)
    print(f"pooled chi-square {stat:.3f}, bound {hi:.3f}")
    assert 38.2 < hi < 38.3
    assert stat < hi


@pytest.fixture(scope="module")
def calibration():
    X, S = ref.calibration_samples()
    return X, S, ref.goodness_of_fit(X, S, 39, seed=0, steps=300)


def test_calibration_of_the_whole_procedure(calibration):
    """64 samples drawn from the catalogue itself, V = 96, T = 2000, B = 39, 300 steps on both sides: the p-values' mean lies in
    [0.3, 0.7] and at most 8 of 64 are <= 0.05.  The replica gives mean 0.582 and 3 of 64."""
    X, S, (obs, drawn, null_errors, n_exceed, mean, p) = calibration
    assert X.shape == (72, 96) and S.shape == (4, 96) and np.array_equal(X.sum(axis=1), np.full(72, 2000.0))
    assert drawn.shape == (39, 72, 96) and np.array_equal(drawn.sum(axis=2), np.full((39, 72), 2000.0))
    assert np.array_equal(p, (1 + n_exceed) / 40)
    null = p[:64]
    print(f"null samples: mean p {null.mean():.3f}, {int((null <= 0.05).sum())} of 64 at or below 0.05")
    assert 0.3 <= null.mean() <= 0.7
    assert (null <= 0.05).sum() <= 8


def test_a_planted_signature_is_rejected(calibration):
    """8 samples with 30 % of their mutations moved to a signature outside the catalogue: no null divergence reaches the
    observed one, p = 1 / 40.  (The replica's observed divergences are 14.9 to 17.6 times the largest null one.)"""
    _, _, (obs, drawn, null_errors, n_exceed, mean, p) = calibration
    ratio = obs.reconstruction_errors[64:] / null_errors[:, 64:].max(axis=0)
    print(f"planted samples: observed / largest null divergence {ratio.min():.2f} .. {ratio.max():.2f}")
    assert np.array_equal(n_exceed[64:], np.zeros(8, dtype=np.int32))
    assert np.array_equal(p[64:], np.full(8, 1 / 40))
    assert np.all(mean[64:] < obs.reconstruction_errors[64:])


def test_reduction_rules():
    err_obs = np.array([1.0, 2.0, np.nan, 0.5])
    err_null = np.array([[1.0, 1.0, 1.0, np.nan], [0.5, 3.0, 1.0, 0.5], [2.0, 2.0, 1.0, 0.75]])
    n_exceed, mean, p = ref.reduce_null(err_obs, err_null)
    assert n_exceed.dtype == np.int32 and n_exceed.tolist() == [2, 2, 0, 2]  # ties count, NaNs on either side do not
    assert mean[0] == (0.0 + 1.0 + 0.5 + 2.0) / 3 and np.isnan(mean[3])
    assert p.tolist() == [3 / 4, 3 / 4, 1 / 4, 3 / 4]


class FakeLibrary:
    """Stands where ``libsalnmf.so`` would: records the calls that get past the validation and fills nothing."""

    def __init__(self):
        self.calls = []

    def salnmf_draw_model_counts(self, *args):
        self.calls.append(("draw", args))
        return 0

    def salnmf_goodness_of_fit(self, *args):
        self.calls.append(("gof", args))
        return 0


def test_refusals_come_before_the_library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(gof_mod._lib, "load_with_device", lambda: fake)
    X, W = refit_ref.poisson_catalogue(4, 3, V=10, seed=0)
    H = np.ones((4, 3))
    totals = X.sum(axis=1)

    def refused(match, call, *args, **kw):
        with pytest.raises(ValueError, match=match):
            call(*args, **kw)
        assert not fake.calls

    gof = sal.goodness_of_fit
    refused("1 to 96 signatures, got 97", gof, X, np.ones((97, 10)))
    refused("1 to 96 features, got 97", gof, np.ones((3, 97)), np.ones((2, 97)))
    refused("integer counts: row 1, column 2 holds 0.5", gof, np.where((np.arange(4)[:, None] == 1) & (np.arange(10) == 2), 0.5, X), W)
    big = X.copy()
    big[2, 0] = 2.0**32 - X[2, 1:].sum()
    refused("row totals below 2\\*\\*32: row 2", gof, big, W)
    refused("'n_draws' must be an integer in \\[1, 65536\\]", gof, X, W, n_draws=0)
    for n_draws in (65537, -1, 2.5, True):
        refused("'n_draws'", gof, X, W, n_draws=n_draws)
    refused("finite and non-negative", gof, -X, W)
    refused("finite and non-negative", gof, np.full_like(X, np.inf), W)
    refused("features", gof, X, np.ones((3, 9)))
    refused("positive sum", gof, X, np.vstack([W[:2], np.zeros((1, 10))]))
    refused("'seed'", gof, X, W, seed=-1)
    refused("min_iterations <= max_iterations", gof, X, W, min_iterations=5, max_iterations=4)
    refused("'conv_test_freq'", gof, X, W, conv_test_freq=0)
    refused("'tol'", gof, X, W, tol=float("nan"))
    refused("'chunk_bytes'", gof, X, W, chunk_bytes=0)

    draw = sal.draw_model_counts
    refused("Exposures must be finite and non-negative", draw, -H, W, totals, 2)
    refused("Exposures must be finite and non-negative", draw, np.where(H == 1, np.nan, H), W, totals, 2)
    refused("Totals must be non-negative integers below 2\\*\\*32", draw, H, W, -totals, 2)
    refused("Totals must be non-negative integers", draw, H, W, totals + 0.5, 2)
    refused("Totals must be non-negative integers", draw, H, W, np.full(4, 2.0**32), 2)
    refused("one trial count per row", draw, H, W, totals[:3], 2)
    refused("samples x 3 signatures", draw, np.ones((4, 2)), W, totals, 2)
    refused("1 to 96 signatures, got 97", draw, np.ones((4, 97)), np.ones((97, 10)), totals, 2)
    refused("1 to 96 features, got 97", draw, H, np.ones((3, 97)), totals, 2)
    refused("'n_draws'", draw, H, W, totals, 0)
    refused("'seed'", draw, H, W, totals, 2, seed=2**64)

    # valid calls get as far as the library, with the arguments in the C order
    out = draw(H, W, totals, 2, seed=7)
    assert out.shape == (2, 4, 10) and fake.calls[-1][0] == "draw" and fake.calls[-1][1][2:4] == (4, 3) and fake.calls[-1][1][7:9] == (2, 7)
    res = gof(X, W, n_draws=5, seed=3, max_iterations=600, keep_draws=True)
    name, args = fake.calls[-1]
    assert name == "gof" and args[2:4] == (4, 10) and args[5:13] == (3, 5, 3, 500, 600, 10, 1e-7, 256 << 20)
    assert res.null_errors.shape == (5, 4) and res.null_n_iterations.shape == (5, 4) and res.draws.shape == (5, 4, 10)
    assert res.n_exceed.dtype == np.int32 and res.p_value.shape == (4,) and res.timings["n_chunks"] == 0
    assert gof(X, W, n_draws=1).draws is None
    assert {"goodness_of_fit", "draw_model_counts", "GofResult"} <= set(sal.__all__) and sal.GofResult is gof_mod.GofResult
