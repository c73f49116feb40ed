"""The host replica of the negative-binomial model draw (tests/_nbdraw_ref.py) against its contract and
against the law it claims, the calibration of the goodness-of-fit test built on it, and every refusal of the new Python functions
on a fake library.  No device."""

import mpmath as mp
import numpy as np
import pytest
from scipy import stats

import _gof_ref as gof_ref
import _kl_ref as kl
import _nbdraw_ref as ref
import salamander_amd as sal
from salamander_amd import nb as nb_mod


# ---------------------------------------------------------------------------------------------- the replica's arithmetic
def test_array_fma_and_logarithm_are_the_scalar_ones():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(1500) * 10.0 ** rng.integers(-8, 8, 1500)
    b = rng.standard_normal(1500)
    c = -a * b * (1 + rng.standard_normal(1500) * 10.0 ** rng.integers(-17, -1, 1500))  # cancellation down to the last bits
    c[:500] = rng.standard_normal(500)
    assert np.array_equal(ref.fma(a, b, c), np.array([kl.fma(x, y, z) for x, y, z in zip(a, b, c)]))
    p = np.concatenate([rng.random(500), 10.0 ** rng.uniform(-100, 10, 500), [1.0, 2.0**-54, 2.0**-106, 720.0, 2.0**31]])
    assert all(kl.log_operand_ok(float(v)) for v in p)
    assert np.array_equal(ref.log_pos(p), np.array([kl.emu_log_pos(v) for v in p]))


def test_exp_and_loggam_against_mpmath():
    """Measured here (recorded in DESIGN.md section 24, not a tolerance of any test): exp within 1.2 ulp-equivalents (1.3e-16
    relative) on [-708, 0]; loggam within 1.9e-13 absolute for x < 200 and 1e-15 relative to max(|log Gamma|, 1) up to 4e9.  The
    assertions are loose sanity bounds."""
    rng = np.random.default_rng(2)
    t = np.concatenate([-rng.random(3000) * 708.0, -rng.random(200) * 1e-3, np.maximum(-37.5 / rng.uniform(0.05, 1.0, 500), -708.0), [0.0, 3.8e-17, -708.0, -709.0, -1e9]])
    got = ref.nb_exp(t)
    assert got[-1] == 0.0 and got[-2] == 0.0 and got[-5] == 1.0
    with mp.workprec(200):
        rel = max(float(abs((mp.mpf(float(g)) - mp.exp(mp.mpf(float(v)))) / mp.exp(mp.mpf(float(v))))) for g, v in zip(got[:-2], t[:-2]))
        x = np.concatenate([np.arange(1.0, 200.0), np.floor(10.0 ** rng.uniform(2, 9.6, 1000))])
        lg = ref.nb_loggam(x)
        want = [mp.loggamma(mp.mpf(float(v))) for v in x]
        absolute = max(float(abs(mp.mpf(float(g)) - w)) for g, w in zip(lg[:199], want[:199]))
        relative = max(float(abs(mp.mpf(float(g)) - w) / max(abs(w), 1)) for g, w in zip(lg, want))
    print(f"exp: largest relative error {rel:.3e}; loggam: {absolute:.3e} absolute below 200, {relative:.3e} relative")
    assert rel < 1e-15 and absolute < 1e-11 and relative < 1e-13


# ---------------------------------------------------------------------------------------------- the contract
def small_case():
    rng = np.random.default_rng(3)
    W = rng.dirichlet(np.ones(7), size=3)
    H = rng.uniform(0.5, 40.0, size=(6, 3))
    H[4] = 0.0
    return H, W, np.array([0.05, 0.5, 1.0, 20.0, 1e4, 1e6])


def test_draw_b_depends_on_nothing_but_its_own_counter_words():
    H, W, alpha = small_case()
    d8, failed = ref.draw_nb_counts(H, W, alpha, 8, seed=7)
    assert failed == 0 and d8.shape == (8, 6, 7) and np.array_equal(d8, np.floor(d8))
    assert np.array_equal(ref.draw_nb_counts(H, W, alpha, 4, seed=7)[0], d8[:4])
    assert np.array_equal(ref.draw_nb_counts(H[[2, 5]], W, alpha[[2, 5]], 8, seed=7, rows=[2, 5])[0], d8[:, [2, 5]])
    assert not np.array_equal(ref.draw_nb_counts(H[[2]], W, alpha[[2]], 1, seed=7)[0][0, 0], d8[0, 2])  # row 2 as row 0
    assert not np.array_equal(ref.draw_nb_counts(H, W, alpha, 1, seed=8)[0][0], d8[0]) and not np.array_equal(d8[0], d8[1])
    assert not d8[:, 4].any()  # Lambda = 0: a zero row, not a failure
    assert len(set(d8[:, 3].sum(axis=1))) > 1  # unconditional
    # the streams are separate: a channel's gamma blocks are not the next channel's, nor the total's, nor the placement's
    g = [ref.gamma(np.array([20.0]), stream, 1, 0, 7)[0][0] for stream in (ref.NB_STREAM, ref.NB_STREAM + 1, ref.NB_STREAM_TOTAL, ref.NB_STREAM_PLACE)]
    assert len(set(g)) == 4
    assert ref.NB_STREAM_TOTAL == ref.NB_STREAM + 0xFF00 and ref.NB_STREAM_PLACE == ref.NB_STREAM + 0xFFFF and ref.NB_STREAM == 0x4E42 << 16
    assert ref.NB_STREAM >> 16 not in (0, 0x5350, 0x474F, 0x5053)  # resampler, split, model draw, presence families


def test_the_attempt_caps_end_every_loop():
    calls = []

    def stub(c0, c1, c2, c3, k0, k1):  # every word all ones: u = 1, so a1 = a2 = 1 (s = 2), log u = 0 to rounding, us = 0
        if np.size(c0):
            calls.append(int(np.asarray(c1).reshape(-1)[0]))
        full = np.full(np.shape(c0), 0xFFFFFFFF, dtype=np.uint64)
        return full, full, full, full

    g, ok = ref.gamma(np.array([20.0, 0.5]), ref.NB_STREAM, 0, 0, 1, philox=stub)
    assert not ok.any() and not g.any() and len(calls) == ref.GAMMA_ATTEMPTS
    del calls[:]
    assert ref.poisson(3.0, 0, 0, 1, philox=stub) == (0, False) and len(calls) == ref.EXPONENTIALS // 2
    del calls[:]
    assert ref.poisson(50.0, 0, 0, 1, philox=stub) == (0, False) and len(calls) == ref.PTRS_ATTEMPTS
    H, W, alpha = small_case()
    out, failed = ref.draw_nb_counts(H, W, alpha, 2, seed=1, philox=stub)
    assert failed == 2 * 5 and not out.any()  # every row with a positive mean fails and is written as zeros; the zero row is no failure


# ---------------------------------------------------------------------------------------------- the law
def pooled_chi2(samples, pmf_of, quantile=1 - 1e-6):
    """(statistic, bound): the observed counts of each value against the expected ones, neighbouring values pooled from below
    until a bin expects at least 5, and the `quantile` of chi2 with (bins - 1) degrees of freedom."""
    samples = np.asarray(samples, dtype=np.int64)
    top = int(samples.max()) + 1
    expected = samples.size * pmf_of(np.arange(top))
    expected = np.append(expected, samples.size - expected.sum())  # the upper tail
    observed = np.append(np.bincount(samples, minlength=top), 0)
    bins_e, bins_o, e, o = [], [], 0.0, 0
    for ev, ov in zip(expected, observed):
        e, o = e + ev, o + ov
        if e >= 5.0:
            bins_e.append(e), bins_o.append(o)
            e, o = 0.0, 0
    bins_e[-1] += e
    bins_o[-1] += o
    bins_e, bins_o = np.array(bins_e), np.array(bins_o)
    return float(((bins_o - bins_e) ** 2 / bins_e).sum()), float(stats.chi2.ppf(quantile, len(bins_e) - 1))


@pytest.mark.parametrize("alpha", [0.5, 20.0])
def test_the_counts_follow_the_negative_binomial(alpha):
    rng = np.random.default_rng(11)
    W = gof_ref.refit_ref.normalize(rng.dirichlet(np.ones(7), size=3))
    h = np.array([[30.0, 12.0, 5.0]])
    P = (h @ W)[0]
    B = 2000
    draws, failed = ref.draw_nb_counts(np.repeat(h, 1, axis=0), W, alpha, B, seed=2024)
    assert failed == 0
    counts = draws[:, 0]
    for v in range(7):
        law = stats.nbinom(alpha, alpha / (alpha + P[v]))
        stat, bound = pooled_chi2(counts[:, v], law.pmf)
        se = np.sqrt((P[v] + P[v] ** 2 / alpha) / B)
        print(f"alpha {alpha}, channel {v}: mean {counts[:, v].mean():.3f} (model {P[v]:.3f}, se {se:.3f}), chi2 {stat:.2f} (bound {bound:.2f})")
        assert stat < bound
        assert abs(counts[:, v].mean() - P[v]) < 5 * se


@pytest.mark.parametrize("lam", [3.7, 9.99, 10.0, 57.3])
def test_the_two_poisson_paths(lam):
    B = 2000
    T = np.array([ref.poisson(lam, 5, b, 99) for b in range(B)])
    assert T[:, 1].all()
    stat, bound = pooled_chi2(T[:, 0], stats.poisson(lam).pmf)
    print(f"Poisson({lam}): mean {T[:, 0].mean():.3f}, chi2 {stat:.2f} (bound {bound:.2f})")
    assert stat < bound and abs(T[:, 0].mean() - lam) < 5 * np.sqrt(lam / B)


# ---------------------------------------------------------------------------------------------- calibration
def test_calibration_and_planted_signature():
    """64 gamma-Poisson samples (alpha = 20, K = 4, V = 96, mu = 2000) and 8 with 30 % of the mean moved to a planted fifth
    signature, B = 39, 300 steps.  Measured: mean p 0.488 over the 64 (2 at or below 0.05), every planted sample at n_exceed = 0;
    the Poisson goodness_of_fit replica on the same 64 gives mean p 0.025 -- it calls overdispersion a misfit."""
    X, S, alpha = ref.calibration_samples()
    res = ref.nb_goodness_of_fit(X, S, alpha, 39, seed=0)
    null = res.p_value[:64]
    poisson_p = gof_ref.goodness_of_fit(X[:64], S, 39, seed=0)[5]
    print(f"NB: mean p {null.mean():.3f}, {int((null <= 0.05).sum())} of 64 at or below 0.05; planted n_exceed {res.n_exceed[64:]}; "
          f"Poisson test on the same samples: mean p {poisson_p.mean():.3f}")
    assert 0.32 <= null.mean() <= 0.68  # 0.5 +- 5 x 0.289 / sqrt(64)
    assert np.array_equal(res.n_exceed[64:], np.zeros(8, dtype=np.int32))
    assert poisson_p.mean() < null.mean()


def test_dispersion_test_inputs_of_the_device_test():
    """What tests/test_gpu_nb_gof.py asserts of the device holds on the replica at data seed 0 (the first seed tried)."""
    c = ref.DISPERSION_TEST
    res = ref.dispersion_test(*ref.dispersion_test_data(), c["grid"], c["B"], seed=0)
    assert res.p_value == 1 / 20 and not res.at_upper_edge
    assert res.dispersion_draws.min() <= 10.0 <= res.dispersion_draws.max() or res.dispersion_draws.min() <= 100.0 <= res.dispersion_draws.max()
    res = ref.dispersion_test(*ref.dispersion_test_data(poisson=True), c["grid"], c["B"], seed=0)
    assert res.at_upper_edge and res.p_value > 0.05


# ---------------------------------------------------------------------------------------------- refusals
class FakeLibrary:
    """Stands where ``libsalnmf.so`` would: records the calls that get past the validation and fills nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("salnmf_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0

        return call


def test_refusals_come_before_the_library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(nb_mod._lib, "load_with_device", lambda: fake)
    X, W = gof_ref.refit_ref.poisson_catalogue(4, 3, V=10, seed=0)
    H = np.ones((4, 3))

    def refused(match, call, *args, **kw):
        with pytest.raises(ValueError, match=match):
            call(*args, **kw)
        assert not fake.calls

    draw, gof, test = sal.draw_nb_counts, sal.nb_goodness_of_fit, sal.dispersion_test
    refused("1 to 96 signatures, got 97", draw, np.ones((4, 97)), np.ones((97, 10)), 20.0, 2)
    refused("1 to 96 features, got 97", draw, H, np.ones((3, 97)), 20.0, 2)
    refused("samples x 3 signatures", draw, np.ones((4, 2)), W, 20.0, 2)
    refused("finite and non-negative", draw, -H, W, 20.0, 2)
    refused("finite and non-negative", draw, np.where(np.eye(4, 3) > 0, np.inf, H), W, 20.0, 2)
    refused("at most 2\\*\\*24: row 1", draw, H * np.array([[1.0], [2.0**23], [1.0], [1.0]]), W, 20.0, 2)
    for bad in (0.0, -1.0, np.inf, np.nan, 2e6, [20.0] * 3, "a"):
        refused("'dispersion'", draw, H, W, bad, 2)
        refused("'dispersion'", gof, X, W, bad)
    for n_draws in (0, 65537, -1, 2.5, True):
        refused("'n_draws'", draw, H, W, 20.0, n_draws)
        refused("'n_draws'", gof, X, W, 20.0, n_draws=n_draws)
        refused("'n_draws'", test, X, W, n_draws=n_draws)
    for seed in (-1, 2**64, 0.5):
        refused("'seed'", draw, H, W, 20.0, 2, seed=seed)
        refused("'seed'", gof, X, W, 20.0, seed=seed)
        refused("'seed'", test, X, W, seed=seed)
    refused("1 to 96 signatures, got 97", gof, X, np.ones((97, 10)), 20.0)
    refused("integer counts: row 1, column 2 holds 0.5", gof, np.where((np.arange(4)[:, None] == 1) & (np.arange(10) == 2), 0.5, X), W, 20.0)
    big = X.copy()
    big[2, 0] = 2.0**24 + 1
    refused("at most 2\\*\\*24: row 2", gof, big, W, 20.0)
    refused("at most 2\\*\\*24", test, big, W)
    refused("finite and non-negative", gof, -X, W, 20.0)
    refused("min_iterations <= max_iterations", gof, X, W, 20.0, min_iterations=10, max_iterations=5)
    refused("'tol'", gof, X, W, 20.0, tol=-1.0)
    refused("'chunk_bytes'", gof, X, W, 20.0, chunk_bytes=0)
    refused("strictly increasing", test, X, W, grid=[10.0, 5.0])
    refused("'dispersion'", test, X, W, grid=[1.0, 2e6])
    refused("integer counts", test, X + 0.5, W)
    refused("'quantiles'", test, X, W, quantiles=(0.5, 1.5))
    refused("booleans", test, X, W, interval=1)

    out = draw(H, W, [1.0, 2.0, 3.0, 4.0], 2, seed=7)
    name, args = fake.calls[-1]
    assert out.shape == (2, 4, 10) and name == "salnmf_draw_nb_counts" and args[2:4] == (4, 3) and args[7:9] == (2, 7)
    res = gof(X, W, 20.0, n_draws=5, seed=3, max_iterations=600, keep_draws=True)
    name, args = fake.calls[-1]
    assert name == "salnmf_nb_goodness_of_fit" and args[2:4] == (4, 10) and args[5] == 3 and args[7:14] == (5, 3, 500, 600, 10, 1e-7, 256 << 20)
    assert res.null_errors.shape == (5, 4) and res.draws.shape == (5, 4, 10) and res.p_value.shape == (4,) and np.array_equal(res.dispersion, np.full(4, 20.0))
    assert gof(X, W, 20.0, n_draws=1).draws is None
    assert {"draw_nb_counts", "nb_goodness_of_fit", "NBGofResult", "dispersion_test", "DispersionTestResult"} <= set(sal.__all__)


def test_a_failed_row_is_an_error(monkeypatch):
    class Failing(FakeLibrary):
        def salnmf_draw_nb_counts(self, *args):
            args[-1][0] = 3
            return 0

    monkeypatch.setattr(nb_mod._lib, "load_with_device", lambda: Failing())
    with pytest.raises(RuntimeError, match="3 drawn rows"):
        sal.draw_nb_counts(np.ones((4, 3)), np.ones((3, 10)), 20.0, 2)
