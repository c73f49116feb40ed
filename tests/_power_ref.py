"""A NumPy replica of ``sal.signature_power`` (``csrc/salnmf_power.h``) -- TESTS ONLY.

Written from the contract, on ``_presence_ref``.  For a tested pair (n, s) with null fit h0 (exactly 0.0 at s), share pi and
alternative draw a:
    planting: S0 = the sum of h0 from 0.0 in ascending k over all K; c = 1.0 - pi; Hp[k] = c * h0[k] off s, Hp[s] = pi * S0 --
    one rounded float64 operation each;
    the draw: ``_presence_ref.draw_row`` from Hp with T = sum(x) trials under the Philox counter (q, 0x50570000 + s, n, a) -- the
    level is not in the counter;
    the draw goes through the presence test's two solves -> t*_a;
    e_a = #{b: t_b >= t*_a} over the pair's null statistics (a NaN compares false); detected iff t*_a is not NaN and
    e_a <= max_exceed, the largest m >= 0 with (1 + m) / (B + 1) <= alpha; n_detected counts them, alt_mean is the sum of t*_a
    from 0.0 in ascending a over A; power = n_detected / A; detection_limit = the smallest share with power >= target.
"""

from types import SimpleNamespace

import numpy as np

import _presence_ref as presence_ref
import _refit_ref as refit_ref

POWER_STREAM = 0x50570000


def plant(h0, s, share):
    """The planted row of one pair -> float64 (K,)."""
    h0 = np.asarray(h0, dtype=np.float64)
    S0 = np.float64(0.0)
    for v in h0:
        S0 = S0 + v
    c = np.float64(1.0) - np.float64(share)
    out = c * h0
    out[s] = np.float64(share) * S0
    return out


def plant_all(null_exposures, test, shares):
    """(L, N, S, K) from the null exposures (N, S, K); NaN rows stay NaN."""
    N, S, K = null_exposures.shape
    out = np.full((len(shares), N, S, K), np.nan)
    for l, share in enumerate(shares):
        for n in range(N):
            for j, s in enumerate(test):
                if not np.isnan(null_exposures[n, j]).all():
                    out[l, n, j] = plant(null_exposures[n, j], s, share)
    return out


def pair_draw(hp, W, T, n, s, a, seed):
    """Alternative draw a of the pair (n, s) from the planted row hp -> float64 counts.  No level in the counter."""
    return presence_ref.draw_row(hp, W, T, n, a, int(seed), POWER_STREAM + int(s)).astype(np.float64)


def draws_from(planted, W, totals, test, tested, n_alt_draws, seed):
    """(L, A, N, S, V): every tested pair's draws from the given planted exposures (L, N, S, K); zeros where untested."""
    L, N, S, _ = planted.shape
    out = np.zeros((L, n_alt_draws, N, S, W.shape[1]), dtype=np.float64)
    for l in range(L):
        for n in range(N):
            for j, s in enumerate(test):
                if tested[n, j]:
                    for a in range(n_alt_draws):
                        out[l, a, n, j] = pair_draw(planted[l, n, j], W, totals[n], n, s, a, seed)
    return out


def max_exceed(alpha, B):
    """The largest m >= 0 with (1 + m) / (B + 1) <= alpha in Python floats, or None."""
    passing = [m for m in range(B + 1) if (1 + m) / (B + 1) <= alpha]
    return passing[-1] if passing else None


def reduce_alt(null_statistics, alt_statistics, m):
    """(alt_n_exceed (L, A, N, S) int32, n_detected (L, N, S) int32, alt_mean (L, N, S)) of (B, N, S) and (L, A, N, S)."""
    L, A = alt_statistics.shape[:2]
    with np.errstate(invalid="ignore"):
        e = (null_statistics[None, None] >= alt_statistics[:, :, None]).sum(axis=2).astype(np.int32)
    detected = ~np.isnan(alt_statistics) & (e <= m)
    mean = np.zeros(alt_statistics.shape[:1] + alt_statistics.shape[2:])
    for a in range(A):
        mean = mean + alt_statistics[:, a]
    return e, detected.sum(axis=1).astype(np.int32), mean / A


def power_of(n_detected, A, tested):
    return np.where(tested[None], n_detected / A, np.nan)


def detection_limit(shares, power, target):
    """(N, S): the smallest share with power >= target, NaN if none (or the pair is untested)."""
    shares = np.asarray(shares, dtype=np.float64)
    out = np.full(power.shape[1:], np.nan)
    for idx in np.ndindex(*out.shape):
        for l in range(len(shares)):
            if power[(l,) + idx] >= target:
                out[idx] = shares[l]
                break
    return out


def binomial_cap(n, p, tail):
    """The smallest c with P(Bin(n, p) > c) < tail."""
    from math import exp, lgamma, log

    below = 0.0
    for k in range(n + 1):
        below += exp(lgamma(n + 1) - lgamma(k + 1) - lgamma(n - k + 1) + k * log(p) + (n - k) * log(1.0 - p))
        if 1.0 - below < tail:
            return k
    return n


def power(counts, signatures, test, shares, n_draws, n_alt_draws, alpha=0.05, target_power=0.8, seed=0, candidates=None, steps=300, presence=None):
    """The whole procedure on the host at a fixed step count (``presence``: a result of ``_presence_ref.presence`` for the same
    arguments, to spare its solves)."""
    X = np.asarray(counts, dtype=np.float64)
    W = refit_ref.normalize(signatures)
    (N, V), K = X.shape, W.shape[0]
    S, L, A = len(test), len(shares), n_alt_draws
    m = max_exceed(alpha, n_draws)
    assert m is not None
    pres = presence if presence is not None else presence_ref.presence(X, W, test, n_draws, seed=seed, candidates=candidates, steps=steps)
    C = presence_ref.candidate_sets(candidates, N, K)
    tested = pres.tested
    planted = plant_all(pres.null_exposures, test, shares)
    kw = dict(min_iterations=steps, max_iterations=steps)
    alt = np.full((L, A, N, S), np.nan)
    for j, s in enumerate(test):
        rows = np.flatnonzero(tested[:, j])
        if not rows.size:
            continue
        C0 = C[rows].copy()
        C0[:, s] = False
        drawn = np.stack([[[pair_draw(planted[l, n, j], W, X[n].sum(), n, s, a, seed) for n in rows] for a in range(A)] for l in range(L)])
        flat = drawn.reshape(-1, V)
        f1 = presence_ref.solve(flat, W, np.tile(C[rows], (L * A, 1)), **kw).reconstruction_errors
        f0 = presence_ref.solve(flat, W, np.tile(C0, (L * A, 1)), **kw).reconstruction_errors
        alt[:, :, rows, j] = (f0 - f1).reshape(L, A, rows.size)
    e, n_detected, mean = reduce_alt(pres.null_statistics, alt, m)
    e[:, :, ~tested], n_detected[:, ~tested], mean[:, ~tested] = 0, 0, np.nan
    pw = power_of(n_detected, A, tested)
    return SimpleNamespace(presence=pres, planted_exposures=planted, alt_statistics=alt, alt_n_exceed=e, n_detected=n_detected, alt_mean=mean,
                           power=pw, detection_limit=detection_limit(shares, pw, target_power), max_exceed=m)
