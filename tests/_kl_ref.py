"""Extended-precision reference of the KL objectives (``salnmf_kernels.h: tile_kl, log_pos_n, log_ratio``; forward modes 0
and 1), the per-sample error units the tests use, float64 restatements of what the device is documented to do, and
bit-exact host emulations of the two hand-written logarithms.

Why not the float64 oracle: ``x log x - x`` and ``p - x log p`` are each ~ ``|x log x|`` and cancel to the entry's KL term,
so on counts of 1e5 .. 1e6 or near-perfect fits the oracle's own per-sample value is good to 1e-10 .. 1e-7 relative only,
and an aggregate ``isclose`` hides a pad lane, a table entry or a coefficient.  Here every sample has its own unit.

``kl_rows(X, W, H, mode, prec)`` -- the per-sample divergence:
  mode 0:  sum_v (x != 0 ? x log x - x - x log p : 0) + p               (``_utils_klnmf.py:41-53``, the objective)
  mode 1:  sum_v xe log(xe / pe) - x + p,  x == 0 -> EPSILON in xe AND pe (``_utils_klnmf.py:58-97``, per sample)
  (the two are the same number: an entry with x = 0 contributes p in both)
* ``prec="mp"``: P from exact products summed with ``mpmath.fsum`` (one rounding at ``DPS`` = 50 digits), logarithms and the
  sum over the features in mpmath at 50 digits: every term is good to 1e-50 of itself, the result to 1e-48 of the unit.
* ``prec="ld"``: everything in ``numpy.longdouble`` (x87 extended, eps = 2^-64): each of the ~(K + 6) V roundings is
  2^-64 of a term the unit contains, NumPy adds pairwise, so the error stays below ``(K + 8) 2^-11`` x 2^-53 unit in the
  worst case and ~1e-3 units in practice (the host test measures 'ld' against 'mp' on every small case).  Used where mpmath
  would take minutes (the 16 400-sample case).

Units (first order: one rounding of a term moves the result by 2^-53 times it):
  u0_n = sum_v [ x max(|log p|, 0.5) + |x log x| + x + p + (K + 1) |p - x| ]
  u1_n = sum_v [ |xe log(xe / pe)| + x + p + (K + 1) |p - x| ]
the last term is the rounding of the K-term product P through dKL/dp = 1 - x / p; it is dropped (``exact_p``) where P is a
single exact product.  Both units also carry (K + 1) 2^-1021 per entry: a subnormal P rounds absolutely, by 2^-1074.  Layouts are the engine's: ``X (N, V)``, ``W (K, V)``, ``H (N, K)``.
"""

from __future__ import annotations

import os
import re
import struct

import mpmath as mp
import numpy as np
from mpmath.libmp import mpf_pos, round_nearest, to_float as _mpf_to_float

DPS = 50
EPSILON = float(np.finfo(np.float32).eps)
EPS64 = 2.0**-53
L = np.longdouble

# The yardstick: the largest error of the float64 restatements below against kl_rows, in units of 2^-53 u, over the
# whole-sample cases of ``whole_cases()`` (tests/test_kl_ref_host.py measures and asserts them; DESIGN.md "Accuracy of
# the KL objectives" has the table).  Mode 0: the split form (constants per lane column, NumPy's log); mode 1: the
# per-entry form.  A device value may be off by SLACK times its mode's constant: the device sums in another order and its
# log_pos is documented at 2.25 units per logarithm against the library's 0.5.  Never tuned on the device.
#   mode 0: 1.0709 at "catalogue V=96 N=16 K=1"   (near 0.33, exact 0.33, floor 0.47, subnormal 0.82)
#   mode 1: 0.5983 at "catalogue V=96 N=16 K=1"   (near 0.12, exact 0, floor 0.38, subnormal 0.55)
ORACLE_RATIO = {0: 1.08, 1: 0.60}
SLACK = 4.0

# documented bounds of salnmf_kernels.h
LOG_POS_REL = 2.5e-16  # |log_pos(p) - log p| <= LOG_POS_REL max(|log p|, 0.5)
LOG_RATIO_ABS, LOG_RATIO_ABS_RANGE, LOG_RATIO_REL = 2e-14, 256.0, 1e-15
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10

_mpf = np.frompyfunc(lambda x: mp.mpf(float(x)), 1, 1)
_float = np.frompyfunc(float, 1, 1)


def to_mp(a) -> np.ndarray:
    return _mpf(np.asarray(a, dtype=np.float64))


def to_float(a) -> np.ndarray:
    return _float(a).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the reference
def product_ld(W, H):
    return np.asarray(H, dtype=np.float64).astype(L) @ np.asarray(W, dtype=np.float64).astype(L)


def product_mp(W, H):
    """P (N, V), object: exact products, one rounding of the sum at the working precision"""
    Wm, Hm = to_mp(W), to_mp(H)
    N, K = Hm.shape
    V = Wm.shape[1]
    out = np.empty((N, V), dtype=object)
    with mp.workprec(2200):  # (a product of two float64 has 106 bits: exact)
        prods = [[[Hm[n, k] * Wm[k, v] for k in range(K)] for v in range(V)] for n in range(N)]
    for n in range(N):
        for v in range(V):
            out[n, v] = mp.fsum(prods[n][v])
    return out


def kl_rows(X, W, H, mode=0, prec="ld"):
    """Per-sample divergences (N,): longdouble array (``prec="ld"``) or object array of mpf (``prec="mp"``)."""
    X = np.asarray(X, dtype=np.float64)
    zero = X == 0
    if prec == "ld":
        P, x = product_ld(W, H), X.astype(L)
        if mode == 0:
            xs = np.where(zero, L(1), x)
            t = np.where(zero, L(0), x * np.log(xs) - x - x * np.log(P)) + P
        else:
            xe, pe = np.where(zero, L(EPSILON), x), np.where(zero, L(EPSILON), P)
            t = xe * np.log(xe / pe) - x + P
        return t.sum(axis=1)
    with mp.workdps(DPS):
        P = product_mp(W, H)
        out = np.empty(X.shape[0], dtype=object)
        eps = mp.mpf(EPSILON)
        for n in range(X.shape[0]):
            terms = []
            for v in range(X.shape[1]):
                x, p = mp.mpf(float(X[n, v])), P[n, v]
                if mode == 0:
                    terms.append((x * mp.log(x) - x - x * mp.log(p) if x != 0 else 0) + p)
                else:
                    xe, pe = (eps, eps) if x == 0 else (x, p)
                    terms.append(xe * mp.log(xe / pe) - x + p)
            out[n] = mp.fsum(terms)
        return out


def units(X, W, H, mode=0, exact_p=False):
    """u0 or u1 per sample, float64 (the unit needs two digits, not sixteen)"""
    X = np.asarray(X, dtype=np.float64)
    P = product_ld(W, H)
    K = np.shape(W)[0]
    x = X.astype(L)
    zero = X == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == 0:
            logterm = x * np.maximum(np.abs(np.log(P)), L(0.5)) + np.where(zero, L(0), np.abs(x * np.log(np.where(zero, L(1), x))))
        else:
            logterm = np.where(zero, L(0), np.abs(x * np.log(np.where(zero, L(1), x) / P)))
    u = logterm + x + P + (0 if exact_p else (K + 1)) * np.abs(P - x)
    u = u + (K + 1) * L(2.0**-1021)  # a subnormal product or partial sum rounds absolutely: 2^-1074 = 2^-53 x 2^-1021 (dKL/dp = 1 at x = 0)
    return u.sum(axis=1).astype(np.float64)


def ratio(got, want, u) -> np.ndarray:
    """|got - want| / (2^-53 u) per sample, the difference taken in the reference's precision"""
    if np.asarray(want).dtype == object:
        d = to_float(abs(to_mp(got) - want))
    else:
        d = np.abs(np.asarray(got, dtype=np.float64).astype(L) - want).astype(np.float64)
    return d / (EPS64 * u)


# ---------------------------------------------------------------------------- float64 restatements of the device's forms
def _product64(W, H):
    # (einsum's own loops, not BLAS: a row's sums do not depend on how many rows there are)
    return np.einsum("nk,kv->nv", np.asarray(H, dtype=np.float64), np.asarray(W, dtype=np.float64))


def split_form(X, W, H, reverse=False):
    """Mode 0 as documented (salnmf_kernels.h above log_pos): per sample and lane column l = v mod 16 the constant
    c = sum (x log x - x) in ascending v (xlogx_lane_kernel), then acc_l = c + sum_{v = l mod 16} (p - x log p), then the sum
    over the 16 lane columns; NumPy's log, every operation rounded once.  ``reverse``: the other feature order (v
    descending inside a lane, lanes descending)."""
    X = np.asarray(X, dtype=np.float64)
    N, V = X.shape
    P = _product64(W, H)
    zero = X == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(zero, 0.0, X * np.log(np.where(zero, 1.0, X)) - X)
        tp = np.where(zero, P, P - X * np.log(P))
    total = np.zeros(N)
    lanes = range(15, -1, -1) if reverse else range(16)
    for l in lanes:
        vs = list(range(l, V, 16))
        if reverse:
            vs = vs[::-1]
        c = np.zeros(N)
        for v in vs:
            c = c + tx[:, v]
        acc = c
        for v in vs:
            acc = acc + tp[:, v]
        total = total + acc
    return total


def entry_form(X, W, H, reverse=False):
    """Mode 1 as the forward kernel states it: per entry ``xe log(xe / pe) - x + p`` (NumPy's log of the rounded quotient),
    summed per lane column and then over the lane columns; ``reverse``: the other feature order."""
    X = np.asarray(X, dtype=np.float64)
    N, V = X.shape
    P = _product64(W, H)
    zero = X == 0
    xe, pe = np.where(zero, EPSILON, X), np.where(zero, EPSILON, P)
    t = xe * np.log(xe / pe) - X + P
    total = np.zeros(N)
    for l in (range(15, -1, -1) if reverse else range(16)):
        vs = list(range(l, V, 16))
        acc = np.zeros(N)
        for v in (vs[::-1] if reverse else vs):
            acc = acc + t[:, v]
        total = total + acc
    return total


def oracle_ratio(X, W, H, mode, exact_p=False, prec="ld"):
    """(worst ratio of the float64 restatement of ``mode`` in both feature orders, reference rows, units)"""
    want, u = kl_rows(X, W, H, mode, prec), units(X, W, H, mode, exact_p)
    form = split_form if mode == 0 else entry_form
    worst = max(float(ratio(form(X, W, H, rev), want, u).max()) for rev in (False, True))
    return worst, want, u


# ---------------------------------------------------------------------------------- the table and the two logarithms
def read_logtab():
    """``kLogTab`` as the header holds it: (inv (256,), lc (256,))"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "salamander_amd", "csrc", "salnmf_logtab.h")
    text = open(path).read()
    body = text[text.index("kLogTab") :]
    vals = [float.fromhex(t) for t in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+", body)]
    assert len(vals) == 512, len(vals)
    a = np.array(vals).reshape(256, 2)
    return a[:, 0].copy(), a[:, 1].copy()


def table_definition():
    """The generator's definition, recomputed: inv_i = 2 RN(1 / c_i), c_i = 1 + (i + 0.5) / 256; lc_i = RN(-log(inv_i))."""
    inv, lc = [], []
    with mp.workprec(300):
        for i in range(256):
            c = mp.mpf(1) + (mp.mpf(i) + mp.mpf("0.5")) / 256
            v = 2.0 * rn(1 / c)
            inv.append(v)
            lc.append(rn(-mp.log(mp.mpf(v))))
    return np.array(inv), np.array(lc)


def rn(v) -> float:
    """an mpf rounded once, to nearest even, to float64"""
    return _mpf_to_float(mpf_pos(mp.mpf(v)._mpf_, 53, round_nearest), strict=True)


def fma(a, b, c) -> float:
    """a b + c evaluated exactly in mpmath and rounded once (operands of the logarithms: no overflow, no subnormal result)"""
    with mp.workprec(4400):
        return rn(mp.mpf(a) * mp.mpf(b) + mp.mpf(c))


def _hi(v) -> int:
    return struct.unpack("<q", struct.pack("<d", v))[0] >> 32  # signed high word, as __double2hiint


def log_pos_ok(v) -> bool:
    return ((_hi(v) - 0x00100000) & 0xFFFFFFFF) < 0x7FE00000


def log_operand_ok(v) -> bool:
    return ((_hi(v) - 0x03D00000) & 0xFFFFFFFF) < (0x7C200000 - 0x03D00000)


def emu_log_pos(p, tab=None) -> float:
    """``log_pos_n`` operation for operation (salnmf_kernels.h): plain products and sums are float64 operations, every fma
    is exact-then-rounded-once.  p positive normal (``log_pos_ok``)."""
    inv, lc = tab if tab is not None else _TAB()
    p = float(p)
    i = (_hi(p) >> 12) & 0xFF
    m, e = np.frexp(p)  # m in [0.5, 1): v_frexp_mant_f64 / v_frexp_exp_i32_f64
    m, kd = float(m), float(e)
    r = fma(m, inv[i], -1.0)
    r2 = r * r
    h = fma(r, 0.2, -0.25)
    h = fma(r, h, 0.33333333333333331)
    h = fma(r, h, -0.5)
    h = fma(r2, h, r)
    u = fma(kd, LN2_HI, lc[i])
    h = fma(kd, LN2_LO, h)
    return u + h


T1 = (0.1365426141372305, 0.15389174135906675, 0.22222223148322984, 0.40000000000009306)
T2 = (0.1320375159044889, 0.18181729869745253, 0.2857142856666864, 0.6666666666666666)


def emu_log_ratio(x, p, t1=T1, t2=T2) -> float:
    """``log_ratio`` operation for operation.  ``div_path`` is emulated as a correctly rounded division (the device's
    reciprocal-and-refine sequence is documented as such; this emulation cannot see a last-bit difference there)."""
    x, p = float(x), float(p)
    hx, hp = _hi(x), _hi(p)
    k = (hx - hp + 0x80000) >> 20
    bits = struct.unpack("<Q", struct.pack("<d", p))[0]
    ps = struct.unpack("<d", struct.pack("<Q", (bits + (k << 52)) & 0xFFFFFFFFFFFFFFFF))[0]  # p 2^k by exponent-field add
    s = (x - ps) / (x + ps)
    z = s * s
    w = z * z
    a = fma(w, fma(w, fma(w, t1[0], t1[1]), t1[2]), t1[3])
    b = fma(w, fma(w, fma(w, t2[0], t2[1]), t2[2]), t2[3])
    R = z * fma(z, a, b)
    kd = float(k)
    t = fma(kd, LN2_LO, s * R)
    t = fma(2.0, s, t)
    return fma(kd, LN2_HI, t)


def log_ratio_flip(k, p=1.0):
    """The two neighbouring float64 x between which the integer estimate of round(log2(x / p)) goes from k to k + 1.  The
    estimate rounds the difference of the HIGH WORDS (exponent and top 20 mantissa bits), so its seam is where that
    difference reaches (k << 20) + 0x80000 -- x = 1.5 x 2^k for p = 1, not sqrt(2) 2^k; |s| stays below 0.2025 either way."""
    hx = _hi(float(p)) + (k << 20) + 0x80000
    at = struct.unpack("<d", struct.pack("<Q", hx << 32))[0]
    return float(np.nextafter(at, 0.0)), at


_tab_cache = []


def _TAB():
    if not _tab_cache:
        _tab_cache.append(read_logtab())
    return _tab_cache[0]


def log_ratio_bound(x, p, exact) -> float:
    """The documented bound on log_ratio's absolute error at (x, p); ``exact`` = log(x / p)."""
    # The comment states the relative bound "away from ratio = 1" and "better than log(fl(x / p)) near it".  This holds the
    # relative bound at EVERY ratio, which is what that sentence amounts to: x - p' is exact (Sterbenz), x + p' and the
    # division round once each, 2 s is exact, s R(s^2) is below 0.03 |2 s| and the last fma rounds once -- under
    # 4 x 2^-53 = 4.4e-16 relative in all (a division good to 1 ulp instead of 0.5 adds 1.1e-16), where log(fl(x / p)) near 1
    # loses 2^-53 / |log|.
    a = abs(float(exact))
    b = LOG_RATIO_REL * a  # (ratio 1: the result is exactly 0)
    if a <= LOG_RATIO_ABS_RANGE:
        b = min(b, LOG_RATIO_ABS)
    return b


# --------------------------------------------------------------------------------------------------------- the probes
def ulp_step(v, j):
    for _ in range(abs(j)):
        v = float(np.nextafter(v, np.inf if j > 0 else 0.0))
    return v


def log_pos_probes(n_random=100000, seed=7):
    """Arguments of log_pos (float64, positive normal), with a label each: both ends of the 256 mantissa intervals +-1 ulp
    at exponents -1022, -1, 0, 1, 1023 (every interval at exponent 0, every 16th elsewhere), p = 1 +- j ulp, and
    ``n_random`` arguments log-uniform over the normal range."""
    out = []
    for e in (0, -1022, -1, 1, 1023):
        for i in range(0, 256, 1 if e == 0 else 16):
            for name, m in (("lo", 1 + i / 256), ("hi", 1 + (i + 1) / 256)):
                for j in (-1, 0, 1):
                    v = ulp_step(float(np.ldexp(m, e)), j) if np.isfinite(np.ldexp(m, e)) else np.inf
                    if np.isfinite(v) and log_pos_ok(v):
                        out.append((v, f"interval {i} {name} end {j:+d} ulp, exponent {e}"))
    for j in range(1, 9):
        out.append((ulp_step(1.0, j), f"1 + {j} ulp"))
        out.append((ulp_step(1.0, -j), f"1 - {j} ulp"))
    rng = np.random.default_rng(seed)
    for t, v in enumerate(np.exp2(rng.uniform(-1022, 1024, n_random))):
        if np.isfinite(v) and v >= 2.0**-1022:
            out.append((float(v), f"random {t}"))
    return out


def log_ratio_probes():
    """(x, p, label): ratio 1 and its neighbourhood, both sides of every seam of the integer estimate of k for k in -3 .. 3
    and at the extremes, operands at and just inside both log_operand_ok boundaries, x = EPSILON against p over 40 decades."""
    out = []
    for base in (1.0, 1234.5, 3e-7, 2.0**40):
        out.append((base, base, f"ratio 1 at {base:g}"))
        out.append((base * (1 + 2.0**-52), base, f"ratio 1 + 2^-52 at {base:g}"))
        out.append((base, base * (1 + 2.0**-52), f"ratio 1 - 2^-52 at {base:g}"))
        for d in (1e-12, 1e-6):
            out.append((base * (1 + d), base, f"ratio 1 + {d:g} at {base:g}"))
            out.append((base * (1 - d), base, f"ratio 1 - {d:g} at {base:g}"))
    for k in (-3, -2, -1, 0, 1, 2, 3, 40, -40, 600, -600):
        for pm in (1.0, 1.2345678901234567, 1.9999999):
            below, at = log_ratio_flip(k, pm)
            out.append((below, pm, f"k seam {k} -> {k + 1} below, p = {pm}"))
            out.append((at, pm, f"k seam {k} -> {k + 1} at, p = {pm}"))
            r2 = float(np.sqrt(2.0)) * 2.0**k * pm
            out.append((ulp_step(r2, -1), pm, f"sqrt(2) 2^{k} - 1 ulp, p = {pm}"))
            out.append((ulp_step(r2, 1), pm, f"sqrt(2) 2^{k} + 1 ulp, p = {pm}"))
    lo, hi = 2.0**-962, float(np.nextafter(2.0**963, 0.0))  # high words 0x03D00000 and 0x7C1FFFFF: first and last operand accepted
    for name, b in (("low", lo), ("high", hi)):
        inside = b * 1.5 if name == "low" else b / 1.5
        for v, tag in ((b, "at"), (inside, "inside")):
            out.append((v, 1.0, f"x {tag} the {name} boundary, p = 1"))
            out.append((1.0, v, f"p {tag} the {name} boundary, x = 1"))
            out.append((v, v * (1.3 if name == "low" else 1 / 1.3), f"x {tag} the {name} boundary, p = x * 1.3^+-1"))
    for d in range(-20, 21):
        out.append((EPSILON, 10.0**d * 1.0000001, f"x = EPSILON, p = 1e{d}"))
    return out


def log_ratio_outside():
    """operands just outside log_operand_ok on each side: the kernel falls back to the library log for the entry"""
    lo, hi = float(np.nextafter(2.0**-962, 0.0)), 2.0**963
    return [(lo, 1.0, "x below the low boundary"), (1.0, lo, "p below the low boundary"), (hi, 1.0, "x at the high boundary (rejected)"),
            (1.0, hi, "p at the high boundary (rejected)"), (lo / 8, lo * 3, "both below the low boundary")]


# ----------------------------------------------------------------------------------------------- whole-sample states
def _steps(X, W, H, n=3):
    from oracle import klnmf_oracle as orc

    Wt, Ht = W.T, H.T
    for _ in range(n):
        Wt, Ht = orc.update_WH(X.T, Wt, Ht)
    return np.ascontiguousarray(Wt.T), np.ascontiguousarray(Ht.T)


def whole_state(kind, V, N, K):
    """(X, W, H, exact_p) of one whole-sample case:
    catalogue   Poisson counts with 10 % of the entries zeroed, after three oracle steps
    near        X = rint(H W) with entries of 1e5 .. 1e6: KL ~ 1 per entry against |x log x| ~ 1e7
    exact       K = 1, W powers of two, X = fl(H W) exactly: the exact KL is 0
    floor       orc.floor_state, at least a quarter of H at EPSILON
    subnormal   the catalogue state with the last sample of every tile empty (x = 0) and its H at 3e-308 / K: P subnormal,
                finite and non-zero, the tile takes the library branch"""
    from oracle import klnmf_oracle as orc

    seed = 1000 * V + 10 * N + K
    rng = np.random.default_rng(seed)
    if kind in ("catalogue", "subnormal"):
        X, W, H = orc.synthetic_problem(V, N, K, seed=seed)
        X = np.where(rng.random(X.shape) < 0.1, 0.0, np.rint(X))
        X[:, 0] = np.maximum(X[:, 0], 1.0)  # (no all-zero sample: K = 1 would put H at 0)
        W, H = _steps(X, W, H)
        if kind == "subnormal":
            X, H = X.copy(), H.copy()
            rows = [min(n0 + 15, N - 1) for n0 in range(0, N, 16)]
            X[rows] = 0.0
            H[rows] = 3e-308 / K
        return X, W, H, False
    if kind == "near":
        W = rng.dirichlet(np.ones(V), size=K)
        H = rng.uniform(1e5, 1e6, (N, K)) * V / K * 1.0
        X = np.rint(H @ W)
        return X, np.ascontiguousarray(W), H, False
    if kind == "exact":
        assert K == 1
        W = np.exp2(-rng.integers(0, 12, (1, V)).astype(np.float64))
        H = rng.uniform(1e3, 1e6, (N, 1))
        return H @ W, W, H, True
    if kind == "floor":
        X, W, H = orc.floor_state(V, max(N, 64), K, seed=seed, steps=60, active=(1, max(1, K // 8)))
        X, H = np.where(X <= EPSILON, 0.0, X)[:N], H[:N]
        return np.ascontiguousarray(X), W, np.ascontiguousarray(H), False
    raise ValueError(kind)


WHOLE_SHAPES = [(V, N, K) for N in (16, 33) for V in (96, 83) for K in (1, 3, 17, 64)] + [(96, 33, 65), (97, 33, 3)]


def whole_cases():
    """(kind, V, N, K) of section (B): every state at every shape it exists at (exact: K = 1; floor: K >= 3)"""
    out = []
    for V, N, K in WHOLE_SHAPES:
        for kind in ("catalogue", "near", "exact", "floor", "subnormal"):
            if (kind == "exact" and K != 1) or (kind == "floor" and K < 3):
                continue
            out.append((kind, V, N, K))
    return out


def subnormal_rows(N):
    return [min(n0 + 15, N - 1) for n0 in range(0, N, 16)]
