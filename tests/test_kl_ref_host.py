"""CPU checks of the KL reference (``tests/_kl_ref.py``): the logarithm table bit for bit against its definition, the
bit-exact emulations of ``log_pos`` and ``log_ratio`` against mpmath within the bounds documented in ``salnmf_kernels.h``, and
the yardstick of the whole-sample GPU tests -- the float64 restatements of the device's two forms against the
extended-precision rows, in units of ``2^-53 u`` (recorded as ``_kl_ref.ORACLE_RATIO``).

Finding recorded here: the comment of ``log_ratio`` used to promise an absolute error of 2e-14 over |log| <= 460.  The
emulation reaches 2.84e-14 at |log| = 416 -- half an ulp of a result in [256, 512), i.e. the final rounding alone -- so the
comment now states the absolute bound over |log| <= 256 and the relative 1e-15 elsewhere; the arithmetic is unchanged."""

import functools
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

import _kl_ref as R


def test_table_equals_its_definition_bit_for_bit():
    inv, lc = R.read_logtab()
    want_inv, want_lc = R.table_definition()
    assert np.array_equal(inv.view(np.uint64), want_inv.view(np.uint64)), np.flatnonzero(inv != want_inv)
    assert np.array_equal(lc.view(np.uint64), want_lc.view(np.uint64)), np.flatnonzero(lc != want_lc)


def test_fma_emulation_rounds_once():
    rng = np.random.default_rng(0)
    for a, b, c in rng.standard_normal((200, 3)) * np.exp2(rng.integers(-30, 30, (200, 3))):
        assert R.fma(a, b, c) == float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))
    assert R.fma(1.0 + 2.0**-30, 1.0 - 2.0**-30, -1.0) == -(2.0**-60)  # (a rounded product would give 0)


def _log_pos_worst(probes, tab=None):
    worst = (0.0, None, None)
    with mp.workprec(140):
        for p, label in probes:
            exact = mp.log(mp.mpf(p))
            err = abs(float(mp.mpf(R.emu_log_pos(p, tab)) - exact))
            r = err / (R.LOG_POS_REL * max(abs(float(exact)), 0.5))
            if r > worst[0]:
                worst = (r, label, p)
    return worst


def test_emulated_log_pos_within_its_documented_bound():
    """Both ends of all 256 mantissa intervals +-1 ulp, exponents -1022, -1, 0, 1, 1023, p = 1 +- j ulp and 1e5 random
    arguments log-uniform over the normal range: ``|log_pos(p) - log p| <= 2.5e-16 max(|log p|, 0.5)``."""
    probes = R.log_pos_probes()
    assert len(probes) > 100000
    r, label, p = _log_pos_worst(probes)
    print(f"\n[kl-ref] log_pos emulation: worst {r:.3f} of the documented bound at '{label}' (p = {p!r})")
    assert r <= 1.0, f"log_pos emulation exceeds 2.5e-16 max(|log p|, 0.5) by {r:.3f} x at '{label}', p = {p!r}"


def _log_ratio_worst(t1=R.T1, t2=R.T2):
    worst = (0.0, None)
    with mp.workprec(140):
        for x, p, label in R.log_ratio_probes():
            assert R.log_operand_ok(x) and R.log_operand_ok(p), label
            exact = mp.log(mp.mpf(x) / mp.mpf(p))
            err = abs(float(mp.mpf(R.emu_log_ratio(x, p, t1, t2)) - exact))
            bound = R.log_ratio_bound(x, p, exact)
            r = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
            if r > worst[0]:
                worst = (r, label)
    return worst


def test_emulated_log_ratio_within_its_documented_bounds():
    """Ratio 1 and its neighbourhood, both sides of the seams of the integer estimate of k (and of sqrt(2) 2^k), operands at
    and just inside both ``log_operand_ok`` boundaries, x = EPSILON against p over 40 decades: absolute 2e-14 over
    |log| <= 256, relative 1e-15 at every ratio (``_kl_ref.log_ratio_bound``: also next to 1, where log(fl(x / p)) is worse);
    exactly 0 at ratio 1."""
    for base in (1.0, 1234.5, R.EPSILON):
        assert R.emu_log_ratio(base, base) == 0.0
    for x, p, label in R.log_ratio_outside():
        assert not (R.log_operand_ok(x) and R.log_operand_ok(p)), label
    lo, hi = 2.0**-962, float(np.nextafter(2.0**963, 0.0))
    assert R.log_operand_ok(lo) and R.log_operand_ok(hi) and R._hi(lo) == 0x03D00000 and R._hi(hi) == 0x7C1FFFFF
    r, label = _log_ratio_worst()
    print(f"\n[kl-ref] log_ratio emulation: worst {r:.3f} of the documented bound at '{label}'")
    assert r <= 1.0, f"log_ratio emulation exceeds its documented bound by {r:.3f} x at '{label}'"


def test_one_ulp_in_a_table_entry_or_a_coefficient_is_seen():
    """The checks above are sharp enough for what they are for: a table entry moved by one ulp fails the table check (by
    construction) and a coefficient of ``log_ratio`` wrong in the 12th digit fails its bound."""
    t2 = (R.T2[0], R.T2[1], R.T2[2], R.T2[3] * (1 + 1e-12))
    r, label = _log_ratio_worst(R.T1, t2)
    assert r > 1.0, (r, label)
    inv, lc = R.read_logtab()
    lc = lc.copy()
    lc[77] = lc[77] * (1 + 3e-15)  # (a dozen ulps: one ulp of lc is below log_pos's own bound, the table check is what sees it)
    probes = [(v, l) for v, l in R.log_pos_probes(0) if l.startswith("interval 77 ") and l.endswith("exponent 0")]
    assert _log_pos_worst(probes, (inv, lc))[0] > 1.0


# ------------------------------------------------------------------------------------ the yardstick of the whole samples
@functools.lru_cache(maxsize=None)
def _measure(kind, V, N, K):
    X, W, H, exact_p = R.whole_state(kind, V, N, K)
    out = {}
    for mode in (0, 1):
        worst, want, u = R.oracle_ratio(X, W, H, mode, exact_p)
        out[mode] = (worst, want, u)
    return X, W, H, exact_p, out


@pytest.mark.parametrize("kind,V,N,K", R.whole_cases())
def test_float64_restatements_stay_within_the_recorded_yardstick(kind, V, N, K):
    X, W, H, exact_p, out = _measure(kind, V, N, K)
    assert np.isfinite(X).all() and (X >= 0).all() and (H > 0).all()
    # the reference's self-consistency: the mode 0 and mode 1 forms are the same number
    u = np.minimum(out[0][2], out[1][2])
    gap = float((np.abs(out[0][1] - out[1][1]).astype(np.float64) / (R.EPS64 * u)).max())
    assert gap < 0.02, f"{kind} V={V} N={N} K={K}: the two extended forms differ by {gap:.3g} units"
    for mode in (0, 1):
        worst = out[mode][0]
        print(f"\n[kl-ref] {kind} V={V} N={N} K={K} mode {mode}: float64 restatement {worst:.4f} x 2^-53 u")
        assert worst <= R.ORACLE_RATIO[mode], f"{kind} V={V} N={N} K={K} mode {mode}: {worst:.4f} exceeds the recorded {R.ORACLE_RATIO[mode]}"
    if kind == "near":
        kl = out[0][1].astype(np.float64)
        assert (kl / out[0][2] < 1e-6).all(), "the near-perfect case became benign"
    if kind == "floor":
        assert np.mean(H <= R.EPSILON) >= 0.25, np.mean(H <= R.EPSILON)
    if kind == "exact":
        assert float(np.abs(out[0][1]).max()) == 0.0
    if kind == "subnormal":
        P = R.product_ld(W, H)[R.subnormal_rows(N)]
        assert (P > 0).all() and (P < 2.0**-1022).all()


@pytest.mark.parametrize("kind,V,N,K", [("catalogue", 83, 16, 3), ("near", 96, 16, 17), ("exact", 96, 16, 1), ("floor", 83, 16, 3)])
def test_long_double_rows_agree_with_mpmath_rows(kind, V, N, K):
    """``kl_rows(prec="ld")`` against ``prec="mp"`` (exact products, fsum, 50 digits): far below one unit, so the long-double
    rows can stand in where mpmath would take minutes."""
    X, W, H, exact_p = R.whole_state(kind, V, N, K)
    for mode in (0, 1):
        ld, exact = R.kl_rows(X, W, H, mode, "ld"), R.kl_rows(X, W, H, mode, "mp")
        u = R.units(X, W, H, mode, exact_p)
        hi = ld.astype(np.float64)
        lo = (ld - hi.astype(R.L)).astype(np.float64)
        with mp.workdps(R.DPS):
            d = R.to_float(abs(R.to_mp(hi) + R.to_mp(lo) - exact))
        r = float((d / (R.EPS64 * u)).max())
        print(f"\n[kl-ref] {kind} V={V} N={N} K={K} mode {mode}: long double against mpmath {r:.2e} units")
        assert r < 0.02, (kind, mode, r)
