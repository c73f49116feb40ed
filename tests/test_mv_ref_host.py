"""The extended-precision reference of the MvNMF W step (``tests/_mv_ref.py``) against the float64 oracle, on the CPU.

Two purposes: the helper is checked against an independent evaluation (the oracle, within the accuracy the oracle can
have: ``eps * kappa`` where the root cancels, ``eps * cond2(S)`` where it does not), and the oracle's own error is
*measured* in those units.  These ratios are the yardstick of ``tests/test_gpu_mv_entrywise.py``: the device may be off
by ``_mv_ref.SLACK`` times the oracle's worst ratio of the regime.  The table is in DESIGN.md.
"""

import mpmath as mp
import numpy as np
import pytest

import _mv_ref as R
from oracle import klnmf_oracle as orc

EPS = R.EPS64


def _oracle_ratio(X, W, H, ref, lam, unit):
    u = ref.update_W_unconstrained(lam)
    # (H as a C-contiguous (K, N) array, the reference's own layout: NumPy sums its rows pairwise then.  From a transposed
    # view the row sums are accumulated in another order and the ratios of regime (b) move by up to 0.04)
    got = orc.update_W_unconstrained(X.T, W.T, np.ascontiguousarray(H.T), lam, ref.delta).T
    err = u.rel_err(got)
    assert not u.clipped.any() and not u.ambiguous.any()
    return u, err, float((err / (EPS * unit(u))).max())


# V, N, K, lam, delta, count scale | mean row sum of H, max rel. error of the oracle, kappa max, max err / (eps kappa)
TABLE_B = [
    ((96, 900, 8, 0.7, 0.3, 1.0), (2.3e5, 1.6e-9, 4.7e7, 0.55)),
    ((96, 3000, 12, 1.0, 1.0, 1.0), (5.0e5, 4.4e-8, 6.4e8, 0.88)),
    ((96, 20000, 30, 1.0, 1.0, 1.0), (1.3e6, 3.0e-8, 5.1e8, 0.72)),
    ((96, 20000, 30, 1e-3, 1.0, 1.0), (1.3e6, 2.2e-5, 5.1e11, 0.67)),
    ((96, 3000, 12, 1.0, 1.0, 1000.0), (5.0e8, 1.9e-5, 6.4e11, 0.90)),
]


@pytest.mark.parametrize("case,want", TABLE_B)
def test_count_dominated_regime_the_oracle_is_good_to_eps_kappa(case, want):
    """Regime (b), b > 0 on every entry: the oracle's error per entry is explained by the subtraction ``root - b`` alone
    (0.55 .. 0.90 eps kappa), it grows with the counts and with 1 / lam, and the two algebraic forms of the root agree to
    1e-25 in the reference itself."""
    V, N, K, lam, delta, scale = case
    X, W, H = R.problem(V, N, K, scale)
    ref = R.MvRef(W, delta, X, H)
    u, err, ratio = _oracle_ratio(X, W, H, ref, lam, lambda u: u.kappa)
    assert (u.b > 0).all()
    forms = R.to_float(abs(u.Wu_raw - u.Wu_alt) / u.Wu_raw).max()
    print(f"\n(b) {case}: mean r {R.to_float(ref.r).mean():.2g}  oracle max err {err.max():.2g}  kappa max {u.kappa.max():.2g}  "
          f"ratio {ratio:.3f}  forms {forms:.1e}")
    assert forms < 1e-25
    rmean, emax, kmax, tab = want
    assert np.isclose(R.to_float(ref.r).mean(), rmean, rtol=0.05) and np.isclose(err.max(), emax, rtol=0.05)
    assert np.isclose(u.kappa.max(), kmax, rtol=0.05)
    assert abs(ratio - tab) < 0.0075  # the recorded table, to two digits
    assert ratio <= R.ORACLE_RATIO["b"] * 1.01


@pytest.mark.parametrize("V,N,K,tab", [(96, 900, 8, 7.1), (96, 917, 17, 6.6), (83, 964, 64, 7.4)])
def test_lam_dominated_regime_the_oracle_is_good_to_eps_cond(V, N, K, tab):
    """Regime (a): lam so large that b < 0 on every entry; nothing cancels, kappa = 1, and the oracle's worst entry is a
    few eps cond2(S) -- the accuracy of A and B (a K-term product with the inverse)."""
    X, W, H = R.problem(V, N, K)
    ref = R.MvRef(W, 1.0, X, H)
    lam = R.lam_dominated(ref)
    u, err, ratio = _oracle_ratio(X, W, H, ref, lam, lambda u: ref.cond)
    print(f"\n(a) {(V, N, K)}: lam {lam:.3g}  cond {ref.cond:.3g}  oracle max err {err.max():.2g}  ratio {ratio:.2f}")
    assert (u.b < 0).all() and (u.kappa == 1).all() and (R.to_float(ref.A) > 0).all() and 1.0 < ref.cond < 2.0
    # (the BLAS kernel of the small products moves a case by up to 10 %; the maximum over the cases holds)
    # (the BLAS kernel decides the order of the K-term products: the cap has the same 15 % of headroom; C_a itself stays
    # 4 x the recorded 7.4)
    assert np.isclose(ratio, tab, rtol=0.15) and ratio <= R.ORACLE_RATIO["a"] * 1.15
    assert err.max() < 1e-14


@pytest.mark.parametrize("delta,duplicates,lam_factor,cond,tab", [(1e-6, "near", 25.0, 9.9e4, 0.025), (1e-10, "near", 25e5, 9.9e8, 0.78),
                                                                  (1e-6, "exact", 25.0, 9.9e4, 0.012), (1e-10, "exact", 25e5, 9.9e8, None)])
def test_ill_conditioned_regime(delta, duplicates, lam_factor, cond, tab):
    """Regime (c): two (near-)duplicate signatures and a tiny delta; cond2(S) = 1e5 / 1e9.  With delta = 1e-10 the rule of
    regime (a) leaves half the entries at b > 0 (A is 1e4 times larger, so the rule gives a smaller lam): a factor 1e5
    more brings every entry to b < 0.  The reference's inverse is checked by its residual."""
    X, W, H = R.problem(96, 900, 8, duplicates=duplicates)
    ref = R.MvRef(W, delta, X, H)
    with mp.workdps(R.DPS):
        res = ref.S @ ref.Y
        for k in range(ref.K):
            res[k, k] -= 1
        assert max(abs(x) for x in res.ravel()) < mp.mpf(10) ** -40
    lam = R.lam_dominated(ref, lam_factor)
    u, err, ratio = _oracle_ratio(X, W, H, ref, lam, lambda u: ref.cond)
    print(f"\n(c) delta {delta} {duplicates}: lam {lam:.3g}  cond {ref.cond:.3g}  oracle max err {err.max():.2g}  ratio {ratio:.4f}")
    assert (u.b < 0).all() and np.isclose(ref.cond, cond, rtol=0.02)
    assert (tab is None or np.isclose(ratio, tab, rtol=0.25)) and ratio <= R.ORACLE_RATIO["c"] * 1.01
    assert ratio <= R.ORACLE_RATIO_C[(delta, duplicates)] * 1.25  # the per-case yardstick of the GPU test
    if delta == 1e-10 and duplicates == "near":  # the rule of regime (a) unchanged: half the entries cancel
        u2 = ref.update_W_unconstrained(R.lam_dominated(ref))
        assert np.isclose((u2.b < 0).mean(), 0.5, atol=0.01)


@pytest.mark.parametrize("V,N,K,delta,duplicates", [(96, 900, 8, 0.3, None), (96, 3000, 12, 1.0, None), (96, 917, 17, 1.0, None),
                                                    (83, 964, 64, 1.0, None), (96, 900, 8, 1e-6, "near"), (96, 900, 8, 1e-10, "near"),
                                                    (96, 900, 8, 1e-6, "exact"), (96, 900, 8, 1e-10, "exact")])
def test_logdet_of_the_oracle_within_the_pivot_bound(V, N, K, delta, duplicates):
    """``volume_logdet`` of the oracle against ``sum log(pivot)`` at 60 digits, in units of ``eps * logdet_scale`` (the
    bound derived from the pivots, ``_mv_ref.MvRef``): at most 0.46."""
    _, W, _ = R.problem(V, N, K, duplicates=duplicates)
    ref = R.MvRef(W, delta)
    ratio = abs(float(ref.logdet - mp.mpf(orc.volume_logdet(W.T, delta)))) / (EPS * ref.logdet_scale)
    print(f"\nlogdet {(V, K, delta, duplicates)}: {float(ref.logdet):.6f}  scale {ref.logdet_scale:.3g}  oracle ratio {ratio:.3f}")
    assert ratio <= R.ORACLE_RATIO["logdet"] * 1.01


def test_reference_flags_entries_at_the_clip_floor():
    """Entries whose exact value falls below EPSILON are clipped to it, entries within 1e-6 of it are flagged."""
    X, W, H = R.clip_problem()
    ref = R.MvRef(W, 1.0, X, H)
    u = ref.update_W_unconstrained(1.0)
    assert u.clipped.sum() >= 3 and not u.ambiguous.any()
    assert all(x == mp.mpf(R.EPSILON) for x in u.Wu[u.clipped])
    want = orc.update_W_unconstrained(X.T, W.T, np.ascontiguousarray(H.T), 1.0, 1.0).T
    assert np.array_equal(want == R.EPSILON, u.clipped)


def test_restated_root_is_the_oracle_bit_for_bit():
    """``_mv_ref.restated_root`` from the oracle's own float64 operands gives the oracle's result bit for bit: it is the
    statement the device is held to in ``test_gpu_mv_entrywise.py``."""
    X, W, H = R.problem(96, 900, 8)
    Ht = np.ascontiguousarray(H.T)
    lam, delta = 0.7, 0.3
    Y = np.linalg.inv(W @ W.T + delta * np.eye(8))
    A, B = (W.T @ np.maximum(0.0, -Y)).T, (W.T @ np.abs(Y)).T
    G = ((X.T / (W.T @ Ht)) @ H).T
    got = R.restated_root(W, A, B, G, Ht.sum(axis=1), lam, 2)
    assert np.array_equal(got, orc.update_W_unconstrained(X.T, W.T, Ht, lam, delta, 2).T)
