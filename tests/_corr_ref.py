"""Extended-precision reference of the dense pieces of correlated NMF, and the cases they are tested on.

TEST INFRASTRUCTURE ONLY.  ``oracle/corrnmf_oracle.py`` restated in ``np.longdouble`` (x87 extended, 64-bit mantissa):
``compute_exposures``, ``update_sample_scalings``, ``update_signature_scalings``, ``compute_aux``, ``poisson_llh`` and the
signature update from aux's numerators (``klnmf_oracle.update_W`` with ``n_given_signatures``).  Used by
``test_corr_ref_host.py`` (CPU: the float64 oracle's own error in the units below -- the constants ``C``) and by
``test_gpu_corr_entrywise.py`` (the device, entry by entry).  DESIGN.md section 8.1.

The logits ``beta_k + alpha_n + <L_k, U_n>`` can cancel (regime (c): terms of 100 .. 300, sum of order 1), so they are
not evaluated with rounded products: every float64 factor is split in two halves of <= 26 bits (Veltkamp), the four
partial products of a pair are then *exact*, and the 2 + 4 dim terms of a logit are added with a compensated (Neumaier)
sum in long double -- error ~ 2^-64 |logit| + 2^-128 A instead of 2^-64 A.  ``np.exp`` / ``np.log`` of a long double
array call ``expl`` / ``logl``; ``gammaln`` has no long double form in SciPy, its sum comes from ``mpmath.loggamma`` at
40 digits over the distinct counts.

Units (first-order bounds, eps = 2^-53; ``A[n, k] = |beta_k| + |alpha_n| + sum_m |L[k, m] U[n, m]|``):

    H[n, k]          relative   eps (1 + A[n, k])
    alpha_n          absolute   eps (1 + |log sum_v x| + |log sum_k e^(beta_k + S_nk)| + max_k (|beta_k| + sum_m |L U|))
    beta_k           absolute   eps (1 + |log first_k| + |log second_k| + max_n (|alpha_n| + sum_m |L U|))   (aux given in float64)
    aux[k, n]        relative   eps (K + V + 2)                                                              (H given in float64)
    updated W[k, v]  relative   eps (N + K + V + 2), to max(W_ref, EPSILON); entries that clip equal EPSILON exactly
    likelihood       absolute   eps sum_{n, v} (|x log p| + p + |gammaln(1 + x)|)

aux and W are sums of terms >= 0, so nothing cancels -- but a bare ``eps`` is not a bound for them: measured in it the
float64 oracle itself is 14 units off (K = 1, where aux[0, n] is a 96-term sum, and 13.7 for W at V = 288).  The missing
term is the length of the sums: ``P[n, v]`` is K products and K - 1 additions (K eps), the ratio, its product with W and
the final product with H one rounding each, the sum over the features V - 1: ``(K + V + 2) eps`` for aux; for W the ratio
(K + 1), the product with H, the sum over the samples (N - 1), the product with W, the row sum (V - 1) and the division:
``(N + K + V + 2) eps``.  Both hold for ANY order of the sums.

Rows of X that are all zero are excluded from this work: the reference itself gives ``log 0`` for their alpha.
"""

from __future__ import annotations

import functools
from types import SimpleNamespace

import mpmath as mp
import numpy as np

from oracle import corrnmf_oracle as co
from oracle import klnmf_oracle as ko

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an extended type on this platform"
EPS64 = 2.0**-53
EPSILON = co.EPSILON

# ------------------------------------------------------------------ the constants of the device test
# The float64 ORACLE's largest error over all cases below, in the units above (measured and asserted by
# test_corr_ref_host.py, which also names the case); the device bound per quantity is SLACK x that (DESIGN.md 5.1's rule:
# the 4 covers another summation order and another exp / log implementation).  Never tuned on the device.
SLACK = 4.0
ORACLE_RATIO = {
    "H": 3.7,  # measured 3.68: (c) N=33 K=64 dim=64 V=96 (a 64-term product of terms of 300, BLAS order)
    "alpha": 1.6,  # measured 1.56: (b) N=33 K=64 dim=33 V=96
    "beta": 1.1,  # measured 1.11: (b) N=33 K=64 dim=64 V=96
    "aux": 0.17,  # measured 0.167: (a) N=17 K=3 dim=2 V=7 (2.0 eps against a unit of 12 eps)
    "W": 0.13,  # measured 0.134: (a) N=17 K=3 dim=2 V=7
    "llh": 1.8,  # measured 1.79: (a) N=32769 K=7 dim=3 V=96
}
C = {q: SLACK * v for q, v in ORACLE_RATIO.items()}


# ------------------------------------------------------------------ logits


def _split(a):
    """float64 a = hi + lo exactly, both halves with at most 26 significant bits (Veltkamp)."""
    a = np.asarray(a, dtype=np.float64)
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi.astype(LD), (a - hi).astype(LD)


def logits(beta, alpha, L, U):
    """``(S, A)``, both ``(N, K)`` long double: ``S = beta_k + alpha_n + <L_k, U_n>`` from exact partial products and a
    compensated sum; ``A`` the sum of the terms' magnitudes.  ``beta`` / ``alpha`` may be ``None`` (term absent)."""
    L, U = np.asarray(L, dtype=np.float64), np.asarray(U, dtype=np.float64)
    N, K = U.shape[0], L.shape[0]
    s, c = np.zeros((N, K), dtype=LD), np.zeros((N, K), dtype=LD)

    def add(t):
        nonlocal s, c
        tt = s + t
        c = c + np.where(np.abs(s) >= np.abs(t), (s - tt) + t, (t - tt) + s)
        s = tt

    A = np.zeros((N, K), dtype=LD)
    if beta is not None:
        b = np.asarray(beta, dtype=np.float64).astype(LD)
        add(np.broadcast_to(b[None, :], (N, K)))
        A = A + np.abs(b)[None, :]
    if alpha is not None:
        a = np.asarray(alpha, dtype=np.float64).astype(LD)
        add(np.broadcast_to(a[:, None], (N, K)))
        A = A + np.abs(a)[:, None]
    Lh, Ll = _split(L)
    Uh, Ul = _split(U)
    for m in range(L.shape[1]):
        for x, y in ((Lh, Uh), (Lh, Ul), (Ll, Uh), (Ll, Ul)):
            add(y[:, m, None] * x[None, :, m])  # exact: <= 52 bits
    A = A + np.abs(U).astype(LD) @ np.abs(L).astype(LD).T
    return s + c, A


# ------------------------------------------------------------------ the dense pieces


def compute_exposures(beta, alpha, L, U):
    """``(H (N, K), unit (N, K))``: ``H = exp(logit)``, relative unit ``eps (1 + A)``."""
    S, A = logits(beta, alpha, L, U)
    return np.exp(S), EPS64 * (1.0 + A)


def update_sample_scalings(X, beta, L, U):
    """``(alpha (N), unit (N))``: ``log sum_v x - log sum_k exp(beta_k + S_nk)``."""
    S, A = logits(beta, None, L, U)
    first = np.log(np.asarray(X, dtype=np.float64).astype(LD).sum(axis=1))
    second = np.log(np.exp(S).sum(axis=1))
    return first - second, EPS64 * (1.0 + np.abs(first) + np.abs(second) + A.max(axis=1))


def update_signature_scalings(aux, alpha, L, U):
    """``(beta (K), unit (K))`` from ``aux (K, N)`` given in float64: ``log sum_n aux - log sum_n exp(alpha_n + S_nk)``."""
    S, A = logits(None, alpha, L, U)
    first = np.log(np.asarray(aux, dtype=np.float64).astype(LD).sum(axis=1))
    second = np.log(np.exp(S).sum(axis=0))
    return first - second, EPS64 * (1.0 + np.abs(first) + np.abs(second) + A.max(axis=0))


def _ratios(X, W, H):
    X, W, H = (np.asarray(a, dtype=np.float64).astype(LD) for a in (X, W, H))
    return X, W, H, X / (H @ W)


def compute_aux(X, W, H):
    """``aux (K, N)`` from ``H`` given in float64; every term is >= 0: relative unit :func:`aux_unit`."""
    X, W, H, R = _ratios(X, W, H)
    return H.T * (W @ R.T)


def update_signatures(X, W, H, n_given):
    """``(W_new (K, V) float64-comparable long double, raw)``: ``raw`` is the normalised update before the given rows are
    restored and the others clipped at EPSILON (what decides whether an entry clips)."""
    X, Wl, H, R = _ratios(X, W, H)
    num = Wl * (H.T @ R)
    raw = num / num.sum(axis=1, keepdims=True)
    new = np.maximum(raw, LD(EPSILON))
    new[:n_given] = Wl[:n_given]
    return new, raw


def gammaln_sums(X):
    """``(sum gammaln(1 + x), sum |gammaln(1 + x)|)`` as long doubles, from mpmath at 40 digits over the distinct values."""
    vals, counts = np.unique(np.asarray(X, dtype=np.float64), return_counts=True)
    with mp.workdps(40):
        terms = [mp.loggamma(mp.mpf(float(v)) + 1) * int(c) for v, c in zip(vals, counts)]
        return to_ld(mp.fsum(terms)), to_ld(mp.fsum(abs(t) for t in terms))


def to_ld(x):
    """mpf -> long double (two float64 pieces)."""
    hi = float(x)
    return LD(hi) + LD(float(x - mp.mpf(hi)))


def poisson_llh(X, W, H, gl=None):
    """``(value, unit)``: ``sum_{P != 0} x log p - sum p - sum gammaln(1 + x)`` with ``P = H W``; ``gl``: a cached
    :func:`gammaln_sums` of X."""
    X, W, H = (np.asarray(a, dtype=np.float64).astype(LD) for a in (X, W, H))
    P = H @ W
    nz = P != 0
    xlogp = np.where(nz, X * np.log(np.where(nz, P, LD(1))), LD(0))
    g, gabs = gammaln_sums(X) if gl is None else gl
    return xlogp.sum() - P.sum() - g, EPS64 * (np.abs(xlogp).sum() + P.sum() + gabs)


# ------------------------------------------------------------------ error measures


def rel_ratio(got, ref, unit):
    """Largest ``|got - ref| / (|ref| unit)`` and where."""
    r = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref) / (np.abs(ref) * unit)
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), tuple(int(j) for j in i)


def abs_ratio(got, ref, unit):
    r = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref) / unit
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), tuple(int(j) for j in i)


def aux_unit(K, V):
    return EPS64 * (K + V + 2)


def w_unit(N, K, V):
    return EPS64 * (N + K + V + 2)


def w_ratio(got, new, raw, n_given, unit, c):
    """The updated W entry by entry: ``(ratio, where, n_clipped)``.  Given rows are not part of the ratio (the caller
    checks them bit for bit); an entry whose raw value lies below EPSILON by more than the bound must equal EPSILON
    exactly (ratio inf otherwise); everything else in units of ``unit max(W_ref, EPSILON)``."""
    got = np.asarray(got, dtype=np.float64)
    r = np.abs(got.astype(LD) - new) / (unit * new)
    clipped = raw < LD(EPSILON) * (1 - c * unit)
    clipped[:n_given] = False
    r = np.where(clipped, np.where(got == EPSILON, 0.0, np.inf), r)
    r[:n_given] = 0.0
    i = np.unravel_index(np.argmax(r), r.shape)
    return float(r[i]), tuple(int(j) for j in i), int(clipped.sum())


# ------------------------------------------------------------------ cases

SHAPES_N = [(n, 5, 3, 96) for n in (1, 15, 16, 17, 63, 64, 65)]  # tile edges of the sample axis
SHAPES_DIM = [(33, 64, d, 96) for d in (1, 3, 4, 5, 16, 17, 32, 33, 48, 49, 64)]  # component masks, the four KSQ classes
SHAPES_K = [(33, k, 2, 96) for k in (1, 4, 5, 16, 17, 32, 33, 47, 48, 49, 64)]  # signature tiles, KP = 16 / 32 / 48 / 64
SHAPES_V = [(17, 3, 2, 7), (33, 18, 5, 83)]  # a short feature axis
SHAPES_BLOCKS = [(33, 5, 2, 97), (40, 18, 5, 288)]  # feature blocks (a second block of one feature; three full blocks)
# The logit kernel runs min(ceil(Np / 64), 2 CUs, 1024) workgroups of four waves, wave w of workgroup b takes the 16-row
# tiles 4 b + w, 4 b + w + 4 grid, ...: as long as the grid is ceil(Np / 64) every wave has at most one tile, so a second
# tile needs Np / 16 > 4 * 2 CUs.  On the MI355X's 256 CUs: 2049 tiles, N = 16 * 2048 + 1 = 32 769 -- wave 0 of workgroup
# 0 then takes tile 0 and the ragged tile 2048 (one live row).  (A device with fewer CUs reaches a second tile earlier.)
SHAPE_TILES = (32769, 7, 3, 96)
SHAPES_A = SHAPES_N + SHAPES_DIM + SHAPES_K + SHAPES_V + SHAPES_BLOCKS + [SHAPE_TILES]
# regimes (b), (c), (d): a ragged tile and more than one workgroup, every KSQ class with a partial last k-step, KP = 32 / 64,
# a short feature axis and feature blocks
SHAPES_SUBSET = [(17, 5, 3, 96), (65, 5, 3, 96), (33, 64, 5, 96), (33, 64, 17, 96), (33, 64, 33, 96), (33, 64, 64, 96),
                 (33, 17, 2, 96), (33, 49, 2, 96), (33, 18, 5, 83), (40, 18, 5, 288)]
CASES = [("a",) + s for s in SHAPES_A] + [(r,) + s for r in "bcd" for s in SHAPES_SUBSET]


def synthetic(N, K, dim, V=96, seed=0):
    """``synthetic()`` of ``test_gpu_corrnmf.py`` (restated: that module needs the engine to import)."""
    rng = np.random.default_rng(seed)
    X, W0, _ = ko.synthetic_problem(V, N, K, seed=seed)
    beta = rng.normal(0.0, 0.3, size=K)
    alpha = np.log(X.sum(axis=1) / K) + rng.normal(0.0, 0.1, size=N)
    L = rng.normal(0.0, 0.5, size=(K, dim))
    U = rng.normal(0.0, 0.5, size=(N, dim))
    return X, W0, beta, alpha, L, U


def inputs(regime, N, K, dim, V):
    """``(X, W, beta, alpha, L, U)`` of a case.

    (a) ordinary: ``synthetic``.
    (b) wide logits: L, U ~ N(0, 1) scaled so that the largest ``|<L_k, U_n>|`` is 160; alpha is the scaling update's
        own value plus noise, so that the row's largest exposure stays at the row's counts and the others fall up to 140
        orders below it.
    (c) cancelling logits: all signature embeddings within 0.3 % of one vector L0, ``<L0, U_n> = -t_n`` with
        ``|t_n|`` in [100, 300] of either sign, ``alpha_n = t_n + log(counts / K) + N(0, 1)``: A is 200 .. 600, the
        logit of order 1 .. 10.
    (d) sparse counts: Poisson counts of sparse exposures, three zero-heavy rows, one row holding a single mutation, one
        feature nobody carries (its column of the updated W clips), exact zeros kept.
    """
    seed = N + K + dim + V
    X, W, beta, alpha, L, U = synthetic(N, K, dim, V, seed=seed)
    rng = np.random.default_rng(seed + 1000 * "abcd".index(regime))
    if regime == "b":
        for attempt in range(64):  # the first draw in which, in some row, one of the first four signatures carries the sum
            L, U = rng.normal(size=(K, dim)), rng.normal(size=(N, dim))  # over k of mode 0 (test_corr_ref_host.py asserts it)
            f = np.sqrt(160.0 / np.abs(L @ U.T).max())
            L, U = L * f, U * f
            if (np.argmax(beta[None, :] + U @ L.T, axis=1) < 4).any():
                break
        alpha = co.update_sample_scalings(X, beta, L, U) + rng.normal(0.0, 0.1, size=N)
    elif regime == "c":
        L0 = rng.normal(size=dim)
        L0 /= np.linalg.norm(L0)
        t = rng.uniform(100.0, 300.0, size=N) * rng.choice([-1.0, 1.0], size=N)
        L = L0[None, :] + rng.normal(0.0, 0.003 / np.sqrt(dim), size=(K, dim))
        U = -t[:, None] * L0[None, :] + rng.normal(0.0, 0.3, size=(N, dim))
        alpha = t + np.log(X.sum(axis=1) / K) + rng.normal(0.0, 1.0, size=N)
    elif regime == "d":
        import _refit_ref

        X, W = _refit_ref.poisson_catalogue(N, K, V=V, seed=seed, mutations=(20, 2000), zero_heavy=min(3, N - 1))
        X[:, V // 3] = 0.0
        if N > 4:
            X[1] = 0.0
            X[1, V // 2] = 1.0
        dead = np.flatnonzero(X.sum(axis=1) == 0)  # (a zero-heavy row whose three mutations all fell on the dead feature)
        X[dead, 0] = 1.0
        alpha = np.log(X.sum(axis=1) / K) + rng.normal(0.0, 0.1, size=N)
    return X, W, beta, alpha, L, U


@functools.lru_cache(maxsize=None)
def case(regime, N, K, dim, V):
    """The inputs of a case and every reference that does not depend on a device result, computed once."""
    X, W, beta, alpha, L, U = inputs(regime, N, K, dim, V)
    c = SimpleNamespace(regime=regime, N=N, K=K, dim=dim, V=V, X=X, W=W, beta=beta, alpha=alpha, L=L, U=U, n_given=K // 3)
    c.H, c.H_unit = compute_exposures(beta, alpha, L, U)
    c.alpha_new, c.alpha_unit = update_sample_scalings(X, beta, L, U)
    c.gl = gammaln_sums(X)
    return c


def tag(regime, N, K, dim, V):
    return f"({regime}) N={N} K={K} dim={dim} V={V}"


# ------------------------------------------------------------------ regime (e): likelihood fallbacks

LLH_SHAPES = [(37, 5, 83), (17, 3, 7), (33, 5, 97)]  # zero rows in a ragged last tile; V = 83, 7; a second feature block


def llh_states(N, K, V):
    """``(X, [(W, H), ...])``, three states of one engine:

    0. two columns of W are 0 (P = 0 there in every row: every tile takes the library-log branch), the last three samples
       have no exposure at all (P = 0 on their rows) and sample 2 has exposures of 3e-308 (its P is subnormal);
    1. the same H with a positive W: only the tiles that hold those samples take that branch;
    2. positive W and H: no such entry, every tile takes the table branch.

    The counts are 0 wherever a P can be 0 (the reference would be -inf otherwise) and not 0 in sample 2."""
    rng = np.random.default_rng(N + K + V)
    X, W, H = ko.synthetic_problem(V, N, K, seed=N + K + V)
    X = np.floor(X)  # (synthetic_problem clips at EPSILON: exact zeros here)
    Wz = W.copy()
    Wz[:, [1, V - 1]] = 0.0
    X[:, [1, V - 1]] = 0.0
    Hz = H.copy()
    Hz[N - 3 :] = 0.0
    X[N - 3 :] = 0.0
    Hz[2] = 3e-308
    X[2] = rng.integers(0, 4, size=V)
    X[2, [1, V - 1]] = 0.0
    return X, [(Wz, Hz), (W, Hz), (W, H)]
