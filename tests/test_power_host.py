"""The power analysis' host side without a device: the replica (tests/_power_ref.py) against its own contract -- the planting,
what a pair's alternative draws depend on, the detection rule, the limit --, the calibration of the whole procedure on the
presence test's null samples, and every argument ``sal.signature_power`` refuses before it touches a device (DESIGN.md
section 18)."""

import math

import numpy as np
import pytest

import _gof_ref as gof_ref
import _power_ref as ref
import _presence_ref as presence_ref
import _refit_ref as refit_ref
import salamander_amd as sal
from salamander_amd import power as power_mod


def small_case(N=6, K=4, V=10, seed=0):
    return refit_ref.poisson_catalogue(N, K, V=V, seed=seed, mutations=(50, 400))


def null_fit(K=17, s=5, seed=2):
    h0 = np.random.default_rng(seed).uniform(1e-3, 300.0, size=K)
    h0[s] = 0.0
    return h0


def test_planting_at_share_zero_returns_the_null_fit():
    for K, s in ((2, 0), (17, 5), (96, 95)):
        h0 = null_fit(K, s)
        assert np.array_equal(ref.plant(h0, s, 0.0), h0) and ref.plant(h0, s, 0.0)[s] == 0.0
    H0 = np.full((3, 2, 4), np.nan)
    H0[0, 0], H0[2, 1] = [0.0, 1.5, 2.5, 1e-30], [3.0, 0.5, 0.0, 7.0]
    planted = ref.plant_all(H0, [0, 2], (0.0, 0.5))
    assert np.array_equal(planted[0], H0, equal_nan=True)  # untested pairs stay NaN
    assert np.array_equal(planted[1, 0, 0], [0.5 * (1.5 + 2.5 + 1e-30), 0.75, 1.25, 0.5e-30]) and np.array_equal(planted[1, 2, 1], [1.5, 0.25, 5.25, 3.5])


def test_the_planted_row_keeps_the_sum():
    """Hp sums to S0 within one rounding per operation: K - 1 additions in S0, the subtraction 1 - pi, one product per entry,
    and the rounding of the exact sum taken here -- (K + 2) u S0 to first order, u = 2**-53."""
    for K, s in ((2, 1), (17, 5), (96, 0)):
        h0 = null_fit(K, s)
        S0 = 0.0
        for v in h0:
            S0 += v
        for share in (0.0, 0.02, 1 / 3, 0.999999):
            hp = ref.plant(h0, s, share)
            assert hp[s] == share * S0 and np.array_equal(np.delete(hp, s), (1.0 - share) * np.delete(h0, s))
            assert abs(math.fsum(hp) - S0) <= 1.01 * (K + 2) * 2.0**-53 * S0, (K, share)


def test_stream_word():
    rng = np.random.default_rng(1)
    W = refit_ref.normalize(rng.dirichlet(np.full(7, 0.5), size=3))
    h = rng.uniform(0.5, 50.0, size=3)
    assert ref.POWER_STREAM == 0x50570000 and ref.POWER_STREAM >> 16 == int.from_bytes(b"PW", "big")
    words = {ref.POWER_STREAM + s for s in range(96)}
    assert not words & ({0, 0x53504C54, gof_ref.GOF_STREAM} | {presence_ref.PRESENCE_STREAM + s for s in range(96)})
    for s in (0, 1, 95):
        mine = ref.pair_draw(h, W, 1000, 4, s, 2, 9)
        assert mine.sum() == 1000 and np.array_equal(mine, ref.pair_draw(h, W, 1000, 4, s, 2, 9))
        assert not np.array_equal(mine, presence_ref.pair_draw(h, W, 1000, 4, s, 2, 9))  # the null draw at the same (seed, n, s, b)
        assert not np.array_equal(mine, gof_ref.draw_row(h, W, 1000, 4, 2, 9))  # the goodness-of-fit draw at the same (seed, n, b)
    for T in (0, 1, 2, 257):
        assert ref.pair_draw(h, W, T, 4, 1, 0, 9).sum() == T


def test_levels_share_their_random_numbers():
    """The level is not in the counter: two levels of a pair have equal draws exactly where their planted rows are equal."""
    X, W = small_case()
    W = refit_ref.normalize(W)
    totals = X.sum(axis=1)
    pres = presence_ref.presence(X, W, [2], 2, seed=5, steps=20)
    planted = ref.plant_all(pres.null_exposures, [2], (0.0, 0.3, 0.6))
    planted[2, 0] = planted[1, 0]  # sample 0: levels 1 and 2 hold the same row
    drawn = ref.draws_from(planted, W, totals, [2], pres.tested, 3, 5)
    assert drawn.shape == (3, 3, 6, 1, 10) and np.array_equal(drawn.sum(axis=4), np.broadcast_to(totals[:, None], (3, 3, 6, 1)))
    assert np.array_equal(drawn[1, :, 0], drawn[2, :, 0])
    for n in range(1, 6):
        assert not np.array_equal(drawn[1, :, n], drawn[2, :, n]) and not np.array_equal(drawn[0, :, n], drawn[1, :, n])
    # a level's draws do not depend on where it stands among the shares
    alone = ref.draws_from(planted[1:2], W, totals, [2], pres.tested, 3, 5)
    assert np.array_equal(alone[0], drawn[1])
    # another s, n, seed or a is another draw
    hp, T = planted[1, 1, 0], totals[1]
    base = ref.pair_draw(hp, W, T, 1, 2, 0, 5)
    assert np.array_equal(base, drawn[1, 0, 1, 0])
    for other in (ref.pair_draw(hp, W, T, 1, 3, 0, 5), ref.pair_draw(hp, W, T, 2, 2, 0, 5), ref.pair_draw(hp, W, T, 1, 2, 0, 6), ref.pair_draw(hp, W, T, 1, 2, 1, 5)):
        assert other.sum() == T and not np.array_equal(other, base)


def test_what_a_pairs_results_depend_on():
    X, W = small_case()
    kw = dict(alpha=0.5, seed=5, steps=30)
    both = ref.power(X, W, [0, 2], (0.0, 0.3), 3, 2, **kw)
    one = ref.power(X, W, [2], (0.3,), 3, 2, **kw)  # not on S, L or the other shares
    more = ref.power(X, W, [2], (0.1, 0.3, 0.5), 3, 4, **kw)  # not on A
    fewer = ref.power(X[:3], W, [2], (0.3,), 3, 2, **kw)  # not on N
    assert both.max_exceed == 1
    for name in ("alt_statistics", "alt_n_exceed"):
        assert np.array_equal(getattr(one, name)[0, :, :, 0], getattr(both, name)[1, :, :, 1]), name
        assert np.array_equal(getattr(one, name)[0], getattr(more, name)[1, :2]), name
        assert np.array_equal(getattr(fewer, name), getattr(one, name)[:, :, :3]), name
    for name in ("n_detected", "alt_mean", "power"):
        assert np.array_equal(getattr(one, name)[0, :, 0], getattr(both, name)[1, :, 1]), name
    assert np.array_equal(one.planted_exposures[0], more.planted_exposures[1])
    assert np.array_equal(both.planted_exposures[0], both.presence.null_exposures)
    # more of the signature, a larger statistic (the same random numbers at every level)
    assert (more.alt_mean[2] > more.alt_mean[0]).all()


def test_max_exceed_is_the_presence_tests_p_value_rule():
    cases = [(0.05, 39), (0.05, 199), (0.05, 200), (0.5, 3), (0.25, 3), (0.1, 9), (0.1, 19), (0.01, 99), (0.01, 999), (1 / 3, 5), (0.3, 9), (0.07, 99),
             (1.0, 7), (0.025, 39)]
    assert any(float(alpha * (B + 1)).is_integer() for alpha, B in cases)
    for alpha, B in cases:
        m = ref.max_exceed(alpha, B)
        assert m is not None and m == power_mod.max_exceed_for(alpha, B)
        for e in range(B + 1):
            assert (e <= m) == ((1 + e) / (B + 1) <= alpha), (alpha, B, e)
    assert ref.max_exceed(0.05, 39) == 1 and ref.max_exceed(0.05, 199) == 9 and ref.max_exceed(0.5, 3) == 1 and ref.max_exceed(0.025, 39) == 0
    for alpha, B in ((0.05, 18), (0.02, 39), (0.0249, 39)):
        assert ref.max_exceed(alpha, B) is None
        with pytest.raises(ValueError, match="cannot be reached"):
            power_mod.max_exceed_for(alpha, B)


def test_reduction_rules():
    null = np.array([0.0, 1.0, 2.0, np.nan])[:, None, None]  # B = 4, one pair
    alt = np.array([[3.0, 2.0, 1.5, np.nan, -1.0]])[:, :, None, None]  # L = 1, A = 5
    e, n_detected, mean = ref.reduce_alt(null, alt, 1)
    assert e.dtype == np.int32 and e[0, :, 0, 0].tolist() == [0, 1, 1, 0, 3]  # ties count, NaNs on either side do not
    assert n_detected.dtype == np.int32 and n_detected[0, 0, 0] == 3  # the NaN draw has e = 0 <= 1 and is not detected
    assert np.isnan(mean[0, 0, 0])
    e, n_detected, mean = ref.reduce_alt(null, alt[:, :3], 0)
    assert n_detected[0, 0, 0] == 1 and mean[0, 0, 0] == (0.0 + 3.0 + 2.0 + 1.5) / 3
    all_nan = np.full((2, 3, 1, 1), np.nan)
    e, n_detected, _ = ref.reduce_alt(null, all_nan, 4)
    assert not e.any() and not n_detected.any()
    tested = np.array([[True]])
    assert np.array_equal(ref.power_of(np.array([[[3]]]), 5, tested), [[[0.6]]]) and np.isnan(ref.power_of(np.array([[[0]]]), 5, ~tested)).all()


def test_detection_limit():
    shares = np.array([0.0, 0.1, 0.2])
    power = np.array([[0.9, 0.05, 0.0, 0.1, np.nan], [1.0, 0.8, 0.5, 0.9, np.nan], [1.0, 1.0, 0.79, 0.7, np.nan]])[:, :, None]
    want = np.array([0.0, 0.1, np.nan, 0.1, np.nan])[:, None]  # the first share passes; exactly the target; none; not monotone; untested
    assert np.array_equal(ref.detection_limit(shares, power, 0.8), want, equal_nan=True)
    assert np.array_equal(power_mod.detection_limit_of(shares, power, 0.8), want, equal_nan=True)
    assert np.array_equal(power_mod.detection_limit_of(shares[:1], power[:1], 0.8), np.array([0.0, np.nan, np.nan, np.nan, np.nan])[:, None], equal_nan=True)


@pytest.fixture(scope="module")
def calibration():
    X, S, s = presence_ref.calibration_samples()
    return ref.power(X[:64], S, [s], (0.0, 0.05, 0.2), 39, 40, alpha=0.05, target_power=0.8, seed=0, steps=300)


def test_power_at_share_zero_sits_near_alpha(calibration):
    """The 64 null samples of the presence test's calibration (T = 2000, four signatures, the fifth tested), B = 39, A = 40,
    alpha = 0.05, 300 steps: the detections at share 0, pooled over 64 * 40 draws, stay at or below the smallest c with
    P(Bin(2560, 0.05) > c) < 1 %, which is 154.  The replica gives 145 (mean power 0.0566): the critical value taken from the
    observed sample's null holds its level here."""
    res = calibration
    pooled = int(res.n_detected[0].sum())
    cap = ref.binomial_cap(64 * 40, 0.05, 0.01)
    print(f"share 0: {pooled} detections of {64 * 40} (cap {cap}), mean power {res.power[0].mean():.4f}; per sample {np.sort(res.n_detected[0, :, 0])}")
    assert res.max_exceed == 1 and cap == 154 and res.presence.tested.all()
    assert pooled <= cap


def test_a_fifth_of_the_mutations_is_detected(calibration):
    """Mean power at share 0.2 is at least the target 0.8.  The replica gives 1.0 there and at share 0.05: every sample's
    detection limit is 0.05."""
    res = calibration
    mean_power = res.power.mean(axis=(1, 2))
    print(f"mean power per share (0, 0.05, 0.2): {mean_power}; detection limits {np.unique(res.detection_limit, return_counts=True)}")
    assert mean_power[2] >= 0.8
    assert (res.alt_mean[2] > res.alt_mean[1]).all() and (res.alt_mean[1] > res.alt_mean[0]).all()


class FakeLibrary:
    """Stands where ``libsalnmf.so`` would: records the calls that get past the validation and fills nothing."""

    def __init__(self):
        self.calls = []

    def salnmf_signature_power(self, *args):
        self.calls.append(args)
        return 0


def test_refusals_come_before_the_library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(power_mod._lib, "load_with_device", lambda: fake)
    X, W = refit_ref.poisson_catalogue(4, 3, V=10, seed=0)

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            sal.signature_power(*args, **kw)
        assert not fake.calls

    # what the presence test refuses
    refused("1 to 96 signatures, got 97", X, np.ones((97, 10)), [0])
    refused("integer counts: row 1, column 2 holds 0.5", np.where((np.arange(4)[:, None] == 1) & (np.arange(10) == 2), 0.5, X), W, [0])
    refused("'test' must be a non-empty list of distinct signature indices in \\[0, 3\\)", X, W, [3])
    refused("'n_draws' must be an integer in \\[1, 65536\\]", X, W, [0], n_draws=0)
    refused("multiple of 'conv_test_freq'", X, W, [0], max_iterations=1005)
    refused("'seed'", X, W, [0], seed=-1)
    refused("'chunk_bytes'", X, W, [0], chunk_bytes=0)
    refused("'candidates' must have shape", X, W, [0], candidates=np.ones((3, 3), dtype=bool))
    # its own
    for shares in ([], (), [1.0], [-0.01], [0.1, 0.1], [0.2, 0.1], [0.0, float("nan")], [float("inf")], [True], ["0.1"], "0.1", 0.1, None, [[0.1]],
                   list(np.arange(65) / 100.0)):
        refused("'shares' must be 1 to 64 strictly ascending numbers in \\[0, 1\\)", X, W, [0], shares=shares)
    for n_alt_draws in (0, 65537, -1, 2.5, True):
        refused("'n_alt_draws' must be an integer in \\[1, 65536\\]", X, W, [0], n_alt_draws=n_alt_draws)
    for alpha in (0.0, -0.1, 1.5, float("nan"), True, "0.05"):
        refused("'alpha' must be a number in \\(0, 1\\]", X, W, [0], alpha=alpha)
    for target in (0.0, 1.01, float("nan"), None):
        refused("'target_power' must be a number in \\(0, 1\\]", X, W, [0], target_power=target)
    refused("'alpha' = 0.05 cannot be reached with 18 null draws", X, W, [0], n_draws=18)
    refused("'alpha' = 0.001 cannot be reached with 200 null draws", X, W, [0], alpha=0.001)

    # a valid call gets as far as the library, with the arguments in the C order
    mask = np.array([True, False, True])
    res = sal.signature_power(X, W, [2, 0], shares=[0.0, 0.5], n_draws=39, n_alt_draws=7, seed=3, candidates=mask, max_iterations=600, keep_draws=True)
    (args,) = fake.calls
    assert args[2:4] == (4, 10) and args[5] == 3 and args[7] == 2 and args[9:16] == (39, 3, 500, 600, 10, 1e-7, 256 << 20) and args[17:20] == (2, 7, 1)
    assert res.max_exceed == 1 and res.alpha == 0.05 and res.target_power == 0.8 and np.array_equal(res.shares, [0.0, 0.5])
    assert res.presence.test == (2, 0) and np.array_equal(res.presence.candidates, np.broadcast_to(mask, (4, 3)))
    for name, shape in (("power", (2, 4, 2)), ("detection_limit", (4, 2)), ("n_detected", (2, 4, 2)), ("alt_mean", (2, 4, 2)),
                        ("planted_exposures", (2, 4, 2, 3)), ("alt_statistics", (2, 7, 4, 2)), ("alt_n_iterations", (2, 7, 4, 2, 2)),
                        ("alt_n_exceed", (2, 7, 4, 2)), ("alt_draws", (2, 7, 4, 2, 10))):
        assert getattr(res, name).shape == shape, name
    for name, shape in (("statistic", (4, 2)), ("null_statistics", (39, 4, 2)), ("null_exposures", (4, 2, 3)), ("draws", (39, 4, 2, 10))):
        assert getattr(res.presence, name).shape == shape, name
    assert np.isnan(res.power).all() and np.isnan(res.detection_limit).all()  # the fake library tested nothing
    assert res.n_detected.dtype == np.int32 and res.alt_n_exceed.dtype == np.int32 and res.timings["n_alt_chunks"] == 0
    quiet = sal.signature_power(X, W, np.array([1]), n_draws=39, n_alt_draws=1)
    assert quiet.alt_draws is None and quiet.presence.draws is None and fake.calls[-1][8] is None and np.array_equal(quiet.shares, [0.0, 0.02, 0.05, 0.1, 0.2])
    assert {"signature_power", "PowerResult"} <= set(sal.__all__) and sal.PowerResult is power_mod.PowerResult
