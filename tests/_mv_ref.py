"""Extended-precision reference of the MvNMF W step (``mvnmf.py:19-24``, ``:37-66``; float64 restatement:
``oracle/klnmf_oracle.py: volume_logdet, update_W_unconstrained``), and the per-entry error measures the tests use.

Why not the float64 oracle: for ``b = r - 4 lam A > 0`` the closed-form root ``W (sqrt(b^2 + 8 lam B G) - b) / (4 lam B)``
subtracts two numbers that agree in their first 6 .. 12 digits, so the oracle's own entries are only good to
``eps * kappa`` with ``kappa = (root + |b|) / (root - b)`` ("Accuracy of the MvNMF W step").  This helper
evaluates the same statements so that its error is far below ``eps`` for every case the tests use:

* everything K- and V-sized in ``mpmath`` at ``DPS`` = 60 digits: ``S = W W^T + delta I``, its inverse ``Y`` and the pivots
  (in-place Gauss-Jordan without pivoting: S is positive definite, and 60 digits leave 50 at cond(S) = 1e9; the host test
  checks ``S Y = I``), ``log det = sum log(pivot)``, ``A = max(0, -Y) W``, ``B = |Y| W``, ``b``, the root and ``Wu``;
* the row sums ``r = sum_n H`` with ``mpmath.fsum`` -- one rounding at 60 digits, i.e. exact for this purpose.  ``r`` is
  the one N-sized quantity whose error the subtraction amplifies by kappa, so it gets no shortcut;
* the numerator ``G = (X / (H W))^T H`` in ``numpy.longdouble`` (x87 extended, eps = 5.4e-20), the contraction over the
  samples in chunks of ``CHUNK`` whose partial sums are then added: the result's relative error is below
  ``(K + CHUNK + N / CHUNK) * 5.4e-20`` < 1e-16 * 0.03 for N <= 40 000 (all terms are positive), and ``G`` enters ``Wu``
  with a sensitivity of at most one (it is not amplified by kappa: ``Wu ~ W G / b`` for ``b > 0``).  mpmath over N V K
  terms would take minutes per case.

Layouts are the engine's: ``X (N, V)``, ``W (K, V)``, ``H (N, K)``; results ``(K, V)``.
"""

from __future__ import annotations

from dataclasses import dataclass

import mpmath as mp
import numpy as np

DPS = 60
CHUNK = 256
EPSILON = float(np.finfo(np.float32).eps)
EPS64 = 2.0**-53
AMBIGUITY = 1e-6  # entries whose exact value lies this close (relative) to EPSILON: the clip's side cannot be decided

# The yardstick: the largest error the float64 oracle itself reaches against this reference, per regime, in units of the
# regime's scale (tests/test_mv_ref_host.py measures and asserts them; DESIGN.md has the table per case):
#   "a"  b < 0 (lam-dominated), well-conditioned S : eps * cond2(S)            (7.4 at K = 64, V = 83)
#   "b"  b > 0 (count-dominated)                    : eps * kappa               (0.90 at counts x 1000)
#   "c"  b < 0, ill-conditioned S                   : eps * cond2(S)            (0.78 at delta = 1e-10)
#   "logdet"                                        : eps * MvRef.logdet_scale  (0.46 at delta = 1e-6)
# A device result may be off by C = SLACK times that: r and G are summed per 16-sample tile and per workgroup slab
# instead of pairwise, and the inverse comes from an elimination without pivoting.  Not tuned on the device.
ORACLE_RATIO = {"a": 7.4, "b": 0.90, "c": 0.78, "logdet": 0.46}
# regime (c) per case (delta, duplicates): the oracle is far better than the regime's maximum on three of the four, and so
# must the device be
ORACLE_RATIO_C = {(1e-6, "near"): 0.029, (1e-10, "near"): 0.78, (1e-6, "exact"): 0.0125, (1e-10, "exact"): 6.3e-7}
SLACK = 4.0
C = {k: SLACK * v for k, v in ORACLE_RATIO.items()}

_mpf = np.frompyfunc(lambda x: mp.mpf(float(x)), 1, 1)
_sqrt = np.frompyfunc(mp.sqrt, 1, 1)
_float = np.frompyfunc(float, 1, 1)


def to_mp(a) -> np.ndarray:
    """float64 array -> object array of exact mpf values"""
    return _mpf(np.asarray(a, dtype=np.float64))


def to_float(a) -> np.ndarray:
    return _float(a).astype(np.float64)


def _invert_spd(S):
    """In-place Gauss-Jordan without pivoting on a copy of the object matrix S: ``(inverse, pivots)``."""
    M = S.copy()
    K = M.shape[0]
    piv = []
    one = mp.mpf(1)
    for k in range(K):
        d = M[k, k]
        piv.append(d)
        M[k, k] = one
        M[k] = M[k] / d
        col = M[:, k].copy()
        col[k] = 0
        M[:, k] = np.where(np.arange(K) == k, M[:, k], 0)
        M -= np.outer(col, M[k])
    return M, piv


@dataclass
class MvWu:
    """``update_W_unconstrained`` at one (lam, n_given) in extended precision, all ``(K, V)``."""

    Wu: np.ndarray  # object (mpf): the exact result, given rows kept, entries below EPSILON clipped
    Wu_raw: np.ndarray  # object: before the clip
    Wu_alt: np.ndarray  # object: the root taken as 8 lam B G / (root + b) where b > 0 (no cancellation)
    b: np.ndarray  # float64
    kappa: np.ndarray  # float64: (root + |b|) / (root - b); 1 where b <= 0
    clipped: np.ndarray  # bool: the exact value lies below EPSILON
    ambiguous: np.ndarray  # bool: the exact value lies within AMBIGUITY of EPSILON
    given: np.ndarray  # bool
    mixed: np.ndarray  # float64: cond2(S) * 4 lam A / |b|, the amplification of A's own error

    def rel_err(self, got) -> np.ndarray:
        """|got - Wu| / Wu per entry, the difference taken in extended precision"""
        return to_float(abs(to_mp(got) - self.Wu) / self.Wu)


class MvRef:
    """Everything of the W step that does not depend on lam: S, Y, cond2(S), log det, A, B (from W and delta), r and G
    (from X, W, H; optional)."""

    def __init__(self, W, delta, X=None, H=None):
        with mp.workdps(DPS):
            W = np.asarray(W, dtype=np.float64)
            self.W, self.delta = W, float(delta)
            self.K, self.V = W.shape
            self.Wm = to_mp(W)
            self.S = self.Wm @ self.Wm.T
            for k in range(self.K):
                self.S[k, k] += mp.mpf(self.delta)
            self.Y, self.pivots = _invert_spd(self.S)
            self.logdet = mp.fsum(mp.log(p) for p in self.pivots)
            ev = np.linalg.eigvalsh(to_float(self.S))
            self.cond = float(ev[-1] / ev[0])
            # scale of the log det's absolute error: pivot k is the Schur complement of the leading block S_k, so it
            # carries a relative error of a few eps * cond2(S_k); log turns that into an absolute error, the K of them
            # add, and so do the roundings of the K logarithms and of their sum (eps * |log pivot| each, eps * |log det|)
            Sf = to_float(self.S)
            conds = [float(np.ptp(e) / e[0] + 1) for e in (np.linalg.eigvalsh(Sf[:k, :k]) for k in range(1, self.K + 1))]
            self.logdet_scale = sum(conds) + float(mp.fsum(abs(mp.log(p)) for p in self.pivots)) + abs(float(self.logdet))
            zero = mp.mpf(0)
            self.A = np.where(self.Y < 0, -self.Y, zero) @ self.Wm
            self.B = abs(self.Y) @ self.Wm
            self.r = self.G = None
            if X is not None:
                self.set_samples(X, H)

    def set_samples(self, X, H):
        X, H = np.asarray(X, dtype=np.float64), np.asarray(H, dtype=np.float64)
        with mp.workdps(DPS):
            self.r = np.array([mp.fsum(H[:, k].tolist()) for k in range(self.K)], dtype=object)
        Wl = self.W.astype(np.longdouble)
        parts = []
        for a in range(0, X.shape[0], CHUNK):
            Hl = H[a : a + CHUNK].astype(np.longdouble)
            parts.append(Hl.T @ (X[a : a + CHUNK].astype(np.longdouble) / (Hl @ Wl)))
        while len(parts) > 1:  # pairwise
            parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        self.G_ld = parts[0]
        hi = self.G_ld.astype(np.float64)
        lo = (self.G_ld - hi.astype(np.longdouble)).astype(np.float64)
        with mp.workdps(DPS):
            self.G = to_mp(hi) + to_mp(lo)
        return self

    def update_W_unconstrained(self, lam, n_given=0) -> MvWu:
        with mp.workdps(DPS):
            lam4 = 4 * mp.mpf(float(lam))
            b = self.r[:, None] - lam4 * self.A
            q = 2 * lam4 * self.B * self.G
            root = _sqrt(b * b + q)
            den = lam4 * self.B
            raw = self.Wm * (root - b) / den
            pos = b > 0
            alt = np.where(pos, self.Wm * (q / (root + np.where(pos, b, 1))) / den, raw)
            kappa = to_float(np.where(pos, (root + abs(b)) / (root - b), 1))
            given = np.zeros((self.K, self.V), dtype=bool)
            given[: int(n_given)] = True
            raw = np.where(given, self.Wm, raw)
            alt = np.where(given, self.Wm, alt)
            eps = mp.mpf(EPSILON)
            clipped = (raw < eps) & ~given
            ambiguous = (to_float(abs(raw / eps - 1)) < AMBIGUITY) & ~given
            mixed = self.cond * to_float(lam4 * self.A / abs(b))
            return MvWu(np.where(clipped, eps, raw), raw, alt, to_float(b), kappa, clipped, ambiguous, given, mixed)

    def line_search_trial(self, Wu, H):
        """``normalize_WH`` + clip of a trial ``Wu`` (object or float, (K, V)): ``(W (K, V) object, column sums)``."""
        with mp.workdps(DPS):
            Wu = Wu if Wu.dtype == object else to_mp(Wu)
            s = np.array([mp.fsum(row) for row in Wu], dtype=object)
            Wn = Wu / s[:, None]
            eps = mp.mpf(EPSILON)
            return np.where(Wn < eps, eps, Wn), s



# ---------------------------------------------------------------------------------------------- the cases of the tests
def problem(V, N, K, scale=1.0, duplicates=None, seed=None):
    """``synthetic_problem(V, N, K, seed=V+N+K)`` after one float64 ``update_H`` (the state the W step sees), counts and
    exposures optionally scaled; ``duplicates``: ``"near"`` makes signatures K-1 and K-2 copies of 0 and 1 up to a relative
    1e-7 of noise, ``"exact"`` exact copies (S is then singular without delta).  Engine layouts."""
    from oracle import klnmf_oracle as orc

    X, W, H0 = orc.synthetic_problem(V, N, K, seed=V + N + K if seed is None else seed)
    if scale != 1.0:
        X, H0 = X * scale, H0 * scale
    if duplicates:
        rng = np.random.default_rng(1)
        W = W.copy()
        for j in range(2):
            W[K - 1 - j] = W[j] * (1.0 if duplicates == "exact" else 1.0 + 1e-7 * rng.standard_normal(V))
            W[K - 1 - j] /= W[K - 1 - j].sum()
    H = np.ascontiguousarray(orc.update_H(X.T, W.T, H0.T).T)
    return X, np.ascontiguousarray(W), H


def lam_dominated(ref: MvRef, factor=25.0) -> float:
    """The lam of regime (a): 4 lam A exceeds the row sums of H everywhere (b < 0), so ``root - b`` adds and kappa = 1."""
    return float(factor * to_float(ref.r).max() / np.median(to_float(ref.A)))


def bound(u: MvWu, ref: MvRef, regime: str, c_neg: float | None = None) -> np.ndarray:
    """The relative error allowed per entry of a device ``Wu``.  b <= 0: ``C eps cond2(S)`` (C of regime "a" or "c").
    b > 0: ``C_b eps kappa`` in regimes "a" / "b"; with an ill-conditioned S (regime "c") ``A`` carries an error of
    ``eps cond2(S)`` of its own, which ``b = r - 4 lam A`` passes on as ``4 lam A / |b|`` and the subtraction amplifies by
    kappa like everything else in b: ``C_b eps kappa (1 + cond2(S) 4 lam A / |b|)`` to first order.  ``c_neg``: the
    constant of the b <= 0 entries where a case has one of its own (``ORACLE_RATIO_C``)."""
    neg = (c_neg if c_neg is not None else C["c" if regime == "c" else "a"]) * EPS64 * ref.cond
    pos = C["b"] * EPS64 * u.kappa * (1.0 + (u.mixed if regime == "c" else 0.0))
    return np.where(u.b > 0, pos, neg)


def clip_problem(V=96, N=900, K=8):
    """A state whose exact W step clips: features 3, 40 and 77 were never observed (zero counts, stored as EPSILON) and
    signature 2 already sits at EPSILON there, so the numerator G is tiny and Wu falls below the floor."""
    from oracle import klnmf_oracle as orc

    X, W, H0 = orc.synthetic_problem(V, N, K, seed=V + N + K)
    X, W = X.copy(), W.copy()
    X[:, [3, 40, 77]] = EPSILON
    W[2, [3, 40, 77]] = EPSILON
    H = np.ascontiguousarray(orc.update_H(X.T, W.T, H0.T).T)
    return X, W, H


def restated_root(W, A, B, G, r, lam, n_given=0):
    """``mv_root_entry`` / ``mvnmf.py:55-65`` in float64, operation for operation (every product and sum rounded once, no
    fused multiply-add), from float64 operands: ``W, A, B, G (K, V)``, ``r (K,)``."""
    lam = float(lam)
    bb = r[:, None] - 4.0 * lam * A
    root = np.sqrt(bb * bb + 8.0 * lam * B * G)
    wu = W * (root - bb) / (4.0 * lam * B)
    wu = np.maximum(wu, EPSILON)
    wu[: int(n_given)] = W[: int(n_given)]
    return wu
