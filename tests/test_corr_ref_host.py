"""The long double reference of CorrNMF's dense pieces (``tests/_corr_ref.py``) on the CPU: the constants of the device test.

For every case of ``test_gpu_corr_entrywise.py`` the float64 ORACLE's largest error against the reference is measured in
the reference's units (module docstring of ``_corr_ref.py``).  ``_corr_ref.ORACLE_RATIO`` records the largest value per
quantity over all cases; the device may be off by ``_corr_ref.SLACK`` = 4 times that.  This file asserts the record (15 %
of headroom: the BLAS kernel of ``L @ U.T`` and of ``H @ W`` decides the second digit), checks the reference itself against
mpmath at 40 digits, and checks the cases: finite everywhere, logits inside (-700, 700), no all-zero row of counts (the
reference itself gives ``log 0`` for such a row's alpha: they are excluded from this work).  Run with ``-s`` for the table
that DESIGN.md section 8.1 quotes.
"""

import functools

import mpmath as mp
import numpy as np
import pytest

import _corr_ref as R
from oracle import corrnmf_oracle as co
from oracle import klnmf_oracle as ko

QUANTITIES = ("H", "alpha", "beta", "aux", "W", "llh")
# the case that set each constant (test_recorded_constants_are_the_measured_maxima)
SET_BY = {
    "H": ("c", 33, 64, 64, 96),
    "alpha": ("b", 33, 64, 33, 96),
    "beta": ("b", 33, 64, 64, 96),
    "aux": ("a", 17, 3, 2, 7),
    "W": ("a", 17, 3, 2, 7),
    "llh": ("a", 32769, 7, 3, 96),
}


@functools.lru_cache(maxsize=None)
def oracle_ratios(*key):
    """The oracle's largest error per quantity on one case, every operation from float64 inputs of its own."""
    c = R.case(*key)
    out = {}
    H64 = co.compute_exposures(c.beta, c.alpha, c.L, c.U)
    out["H"] = R.rel_ratio(H64, c.H, c.H_unit)[0]
    out["alpha"] = R.abs_ratio(co.update_sample_scalings(c.X, c.beta, c.L, c.U), c.alpha_new, c.alpha_unit)[0]
    aux64 = co.compute_aux(c.X, c.W, H64)
    out["aux"] = R.rel_ratio(aux64, R.compute_aux(c.X, c.W, H64), R.aux_unit(c.K, c.V))[0]
    beta, unit = R.update_signature_scalings(aux64, c.alpha, c.L, c.U)
    out["beta"] = R.abs_ratio(co.update_signature_scalings(aux64, c.alpha, c.L, c.U), beta, unit)[0]
    new, raw = R.update_signatures(c.X, c.W, H64, c.n_given)
    out["W"] = R.w_ratio(ko.update_W(c.X.T, c.W.T, H64.T, n_given_signatures=c.n_given).T, new, raw, c.n_given, R.w_unit(c.N, c.K, c.V), R.C["W"])[0]
    llh, unit = R.poisson_llh(c.X, c.W, H64, c.gl)
    out["llh"] = abs(float(R.LD(co.poisson_llh(c.X.T, c.W.T, H64.T)) - llh)) / float(unit)
    return out


@functools.lru_cache(maxsize=None)
def oracle_llh_ratios(N, K, V):
    X, states = R.llh_states(N, K, V)
    gl = R.gammaln_sums(X)
    out = []
    for W, H in states:
        llh, unit = R.poisson_llh(X, W, H, gl)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(abs(float(R.LD(co.poisson_llh(X.T, W.T, H.T)) - llh)) / float(unit))
    return out


@pytest.mark.parametrize("key", R.CASES, ids=lambda k: R.tag(*k))
def test_case_is_sound_and_the_oracle_within_the_record(key):
    c = R.case(*key)
    for name in ("X", "W", "beta", "alpha", "L", "U", "H", "H_unit", "alpha_new", "alpha_unit"):
        assert np.isfinite(np.asarray(getattr(c, name), dtype=np.float64)).all(), name
    assert (c.X.sum(axis=1) > 0).all() and (c.X >= 0).all() and (c.W >= 0).all()
    for b, a in ((c.beta, c.alpha), (c.beta, None), (None, c.alpha)):  # the logits of modes 1, 0, 2
        S, _ = R.logits(b, a, c.L, c.U)
        assert float(np.abs(S).max()) < 700.0
    S, A = R.logits(c.beta, c.alpha, c.L, c.U)
    span = float((S.max(axis=1) - S.min(axis=1)).max())
    if c.regime == "b":
        # wide: some row's exposures span > 100 orders (K > 5: with five signatures the widest row spans fewer), and in some
        # row one of the first four signatures carries the sum of mode 0 (what a loop that skips them must lose)
        assert span > (230.0 if c.K > 5 else 100.0), span
        S0, _ = R.logits(c.beta, None, c.L, c.U)
        assert (np.argmax(S0, axis=1) < 4).any()
    if c.regime == "c":
        assert float(A.min()) > 190.0 and float(np.abs(S).max()) < 25.0 and float(np.abs(c.alpha).min()) > 90.0
    if c.regime == "d":
        assert (c.X == 0).mean() > 0.1 and ((c.X > 0).sum(axis=1) <= 3).sum() >= min(3, c.N - 1) and (c.X.sum(axis=1) == 1).any() and (c.X.sum(axis=0) == 0).any()
    got = oracle_ratios(*key)
    print(f"\n[corr-ref] {R.tag(*key)}: oracle ratios " + "  ".join(f"{q} {got[q]:.3f}" for q in QUANTITIES))
    for q in QUANTITIES:
        assert np.isfinite(got[q]) and got[q] <= R.ORACLE_RATIO[q] * 1.15, (q, got[q])


@pytest.mark.parametrize("N,K,V", R.LLH_SHAPES)
def test_likelihood_fallback_states(N, K, V):
    X, states = R.llh_states(N, K, V)
    tiny = np.finfo(np.float64).tiny
    for i, (W, H) in enumerate(states):
        P = H @ W
        assert (X[P == 0] == 0).all()
        sub = (P > 0) & (P < tiny)
        assert ((P == 0).any() and sub.any() and (X[sub] > 0).any()) if i < 2 else (P >= tiny).all()
    assert (states[0][1][N - 3 :] == 0).all() and (N - 1) // 16 == (N + 15) // 16 - 1 and N % 16 != 0  # zero rows in a ragged last tile
    got = oracle_llh_ratios(N, K, V)
    print(f"\n[corr-ref] (e) N={N} K={K} V={V}: oracle llh ratios " + "  ".join(f"{r:.4f}" for r in got))
    assert max(got) <= R.ORACLE_RATIO["llh"] * 1.15


def test_recorded_constants_are_the_measured_maxima():
    """``_corr_ref.ORACLE_RATIO`` is the largest ratio over all cases, to two digits, and ``C`` four times that."""
    worst = {q: (0.0, None) for q in QUANTITIES}
    for key in R.CASES:
        got = oracle_ratios(*key)
        for q in QUANTITIES:
            if got[q] > worst[q][0]:
                worst[q] = (got[q], key)
    for shape in R.LLH_SHAPES:
        r = max(oracle_llh_ratios(*shape))
        if r > worst["llh"][0]:
            worst["llh"] = (r, ("e",) + shape)
    print("\n[corr-ref] oracle maxima: " + "  ".join(f"{q} {worst[q][0]:.3f} at {worst[q][1]}" for q in QUANTITIES))
    for q in QUANTITIES:
        assert np.isclose(worst[q][0], R.ORACLE_RATIO[q], rtol=0.15), (q, worst[q])
        assert worst[q][0] < 8.0, f"{q}: the oracle is {worst[q][0]:.1f} units off -- the unit is missing a term"
        assert R.C[q] == 4.0 * R.ORACLE_RATIO[q]
        # (the recorded case reaches the maximum; a runner-up within the BLAS kernel's second digit may overtake it)
        at = max(oracle_llh_ratios(*SET_BY[q][1:])) if SET_BY[q][0] == "e" else oracle_ratios(*SET_BY[q])[q]
        assert at >= worst[q][0] / 1.15, (q, worst[q], at)


# ------------------------------------------------------------------ the reference itself against mpmath


def _mp_reference(c):
    """Every quantity of a small case at 40 digits, from the same float64 inputs (aux, W, likelihood from float64(H))."""
    with mp.workdps(40):
        f = lambda a: [[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(a)]
        X, W, L, U = f(c.X), f(c.W), f(c.L), f(c.U)
        beta, alpha = [mp.mpf(float(x)) for x in c.beta], [mp.mpf(float(x)) for x in c.alpha]
        N, K, V, dim = c.N, c.K, c.V, c.dim
        S = [[mp.fsum(L[k][m] * U[n][m] for m in range(dim)) for k in range(K)] for n in range(N)]
        H = [[mp.exp(beta[k] + alpha[n] + S[n][k]) for k in range(K)] for n in range(N)]
        alpha_new = [mp.log(mp.fsum(X[n])) - mp.log(mp.fsum(mp.exp(beta[k] + S[n][k]) for k in range(K))) for n in range(N)]
        H64 = f(np.asarray(c.H, dtype=np.float64))
        P = [[mp.fsum(H64[n][k] * W[k][v] for k in range(K)) for v in range(V)] for n in range(N)]
        aux = [[H64[n][k] * mp.fsum(W[k][v] * X[n][v] / P[n][v] for v in range(V)) for n in range(N)] for k in range(K)]
        aux64 = f(np.array([[float(x) for x in row] for row in aux]))
        beta_new = [mp.log(mp.fsum(aux64[k])) - mp.log(mp.fsum(mp.exp(alpha[n] + S[n][k]) for n in range(N))) for k in range(K)]
        num = [[W[k][v] * mp.fsum(H64[n][k] * X[n][v] / P[n][v] for n in range(N)) for v in range(V)] for k in range(K)]
        raw = [[num[k][v] / mp.fsum(num[k]) for v in range(V)] for k in range(K)]
        llh = mp.fsum(X[n][v] * mp.log(P[n][v]) - P[n][v] - mp.loggamma(X[n][v] + 1) for n in range(N) for v in range(V))
        return H, alpha_new, aux, beta_new, raw, llh


def _worst(got, want, floor=0.0):
    """Largest ``|got - want| / max(|want|, floor)`` of a long double array against nested mpf lists."""
    got, want = np.asarray(got), np.array(want, dtype=object)
    assert got.shape == want.shape
    with mp.workdps(40):
        return float(max(abs(R_ - w) / max(abs(w), mp.mpf(floor)) for R_, w in zip(_as_mp(got.ravel()), want.ravel())))


def _as_mp(values):
    # a long double as the exact sum of two float64 pieces
    for v in values:
        hi = float(v)
        yield mp.mpf(hi) + mp.mpf(float(v - R.LD(hi)))


@pytest.mark.parametrize("regime", ["a", "c"])
def test_reference_agrees_with_mpmath_at_40_digits(regime):
    """< 1e-17 relative on an ordinary and a cancelling case (the scalings, whose units are absolute, relative to
    max(|value|, 1)): the float64 oracle's own error is 1e-16 .. 1e-14 in these quantities."""
    N, K, dim, V = 6, 3, 2, 7
    c = R.case(regime, N, K, dim, V)
    H, alpha_new, aux, beta_new, raw, llh = _mp_reference(c)
    H64 = np.asarray(c.H, dtype=np.float64)
    got_aux = R.compute_aux(c.X, c.W, H64)
    aux64 = np.array([[float(x) for x in row] for row in aux])
    errs = {
        "H": _worst(c.H, H),
        "alpha": _worst(c.alpha_new, alpha_new, 1.0),
        "aux": _worst(got_aux, aux),
        "beta": _worst(R.update_signature_scalings(aux64, c.alpha, c.L, c.U)[0], beta_new, 1.0),
        "W": _worst(R.update_signatures(c.X, c.W, H64, 0)[1], raw),
        "llh": _worst(np.array([R.poisson_llh(c.X, c.W, H64, c.gl)[0]]), [llh]),
    }
    print(f"\n[corr-ref] long double against mpmath, regime ({regime}): " + "  ".join(f"{q} {e:.1e}" for q, e in errs.items()))
    assert max(errs.values()) < 1e-17, errs
    if regime == "c":  # rounded products and a plain long double sum would not do here: the terms are 100 .. 300
        _, A = R.logits(c.beta, c.alpha, c.L, c.U)
        assert float(A.min()) > 190.0


def test_transcendentals_of_a_long_double_stay_long_double():
    x = R.LD(1) / R.LD(3)
    for fn in (np.exp, np.log):
        y = fn(np.array([x]))
        assert y.dtype == R.LD and abs(float(y[0] - R.LD(fn(float(x))))) > 0.0  # (differs from the float64 value: more digits)
    with mp.workdps(40):
        assert abs(next(_as_mp(np.exp(np.array([x])))) - mp.exp(mp.mpf(1) / 3)) < mp.mpf(10) ** -18
        g, _ = R.gammaln_sums(np.array([[0.0, 3.0, 3.0, 1.1920928955078125e-07]]))
        want = 2 * mp.loggamma(4) + mp.loggamma(mp.mpf(1.1920928955078125e-07) + 1)
        assert abs(next(_as_mp([g])) - want) < mp.mpf(10) ** -18
