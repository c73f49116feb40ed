"""A NumPy replica of ``sal.signature_presence_test`` (``csrc/salnmf_presence.h``) -- TESTS ONLY.

Written from the contract.  For sample n with candidate set C and tested signature s in C, |C| >= 2:
    a solve on a set A is ``_assign_masks_ref.assign(x, W, candidates=A, required=A)``: h_k = sum(x) / |A| on A, 0.0 off it, the
    refit's step, objective and stop rule, no elimination (every member is required);
    alternative: the solve on C -> h1, f1;  null: the solve on C \\ {s} -> h0, f0;  statistic = f0 - f1;
    null draw b: the model draw of ``_gof_ref`` (weights, 128-bit product, placement) from h0 with T = sum(x) trials under the
    Philox counter (q, 0x50530000 + s, n, b); the draw goes through the same two solves -> t_b;
    n_exceed = #{b: t_b >= statistic} (a NaN compares false), null_mean = the sum of t_b from 0.0 in ascending b, over B.
Pairs with s outside C or C = {s} are untested: NaN, nothing drawn.
"""

from types import SimpleNamespace

import numpy as np

import _assign_masks_ref as masks_ref
import _gof_ref as gof_ref
import _refit_ref as refit_ref
from _resample_ref import philox4x32_10

PRESENCE_STREAM = 0x50530000
EPSILON = refit_ref.EPSILON


def draw_row(h, W, T, n, b, seed, stream, chunk=1 << 20):
    """One row of one model draw under the second counter word ``stream`` -> int64 counts (``_gof_ref.draw_row`` is this with
    the goodness-of-fit word)."""
    V = np.asarray(W).shape[1]
    out = np.zeros(V, dtype=np.int64)
    T = int(T)
    table = gof_ref.weights(h, W)
    if T == 0 or table is None:
        return out
    cum = table[1]
    M = int(cum[-1])
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    n_blocks = (T + 1) // 2
    for first in range(0, n_blocks, chunk):
        q = np.arange(first, min(first + chunk, n_blocks), dtype=np.uint64)
        o0, o1, o2, o3 = philox4x32_10(q, np.full_like(q, stream), np.full_like(q, n), np.full_like(q, b), k0, k1)
        ulo = np.stack([o0, o2], axis=1).reshape(-1)  # draws 2q, 2q + 1
        uhi = np.stack([o1, o3], axis=1).reshape(-1)
        keep = 2 * int(q[0]) + np.arange(len(ulo)) < T
        t = gof_ref.mulhi(ulo[keep], uhi[keep], M)
        out += np.bincount(np.searchsorted(cum, t, side="right"), minlength=V)
    return out


def pair_draw(h0, W, T, n, s, b, seed):
    """Null draw b of the pair (n, s) from the null fit's exposures h0 -> float64 counts."""
    return draw_row(h0, W, T, n, b, int(seed), PRESENCE_STREAM + int(s)).astype(np.float64)


def draws_from(null_exposures, W, totals, test, tested, n_draws, seed):
    """(B, N, S, V): every tested pair's draws from the given null exposures (N, S, K); zeros where the pair is untested."""
    N, S, _ = null_exposures.shape
    out = np.zeros((n_draws, N, S, W.shape[1]), dtype=np.float64)
    for n in range(N):
        for j, s in enumerate(test):
            if tested[n, j]:
                for b in range(n_draws):
                    out[b, n, j] = pair_draw(null_exposures[n, j], W, totals[n], n, s, b, seed)
    return out


def candidate_sets(candidates, N, K):
    return np.ones((N, K), dtype=bool) if candidates is None else np.broadcast_to(np.asarray(candidates, dtype=bool), (N, K)).copy()


def tested_pairs(C, test):
    """(N, S) bool: s is in the sample's set and not alone in it."""
    return C[:, list(test)] & (C.sum(axis=1) > 1)[:, None]


def solve(X, W, A, **kw):
    """The solve of every row of X on its own row of the (P, K) sets A."""
    return masks_ref.assign(X, W, candidates=A, required=A, **kw)


def reduce_null(statistic, null_statistics):
    """(n_exceed, null_mean, p_value) of (N, S) and (B, N, S) by the stated rules; NaN p where the statistic is NaN."""
    B, N, S = null_statistics.shape
    n_exceed, mean, _ = gof_ref.reduce_null(statistic.reshape(-1), null_statistics.reshape(B, -1))
    n_exceed, mean = n_exceed.reshape(N, S), mean.reshape(N, S)
    return n_exceed, mean, np.where(np.isnan(statistic), np.nan, (1 + n_exceed.astype(np.int64)) / (B + 1))


def presence(counts, signatures, test, n_draws, seed=0, candidates=None, steps=300):
    """The whole procedure on the host at a fixed step count."""
    X = np.asarray(counts, dtype=np.float64)
    W = refit_ref.normalize(signatures)
    (N, V), K = X.shape, W.shape[0]
    S, B = len(test), n_draws
    C = candidate_sets(candidates, N, K)
    tested = tested_pairs(C, test)
    kw = dict(min_iterations=steps, max_iterations=steps)
    nan = np.nan
    statistic, null_errors = np.full((N, S), nan), np.full((N, S), nan)
    null_exposures, null_statistics = np.full((N, S, K), nan), np.full((B, N, S), nan)
    exposures, errors = np.full((N, K), nan), np.full(N, nan)
    rows = np.flatnonzero(tested.any(axis=1))
    if rows.size:
        alt = solve(X[rows], W, C[rows], **kw)
        exposures[rows], errors[rows] = alt.exposures, alt.reconstruction_errors
    for j, s in enumerate(test):
        rows = np.flatnonzero(tested[:, j])
        if not rows.size:
            continue
        C0 = C[rows].copy()
        C0[:, s] = False
        null = solve(X[rows], W, C0, **kw)
        null_exposures[rows, j], null_errors[rows, j] = null.exposures, null.reconstruction_errors
        statistic[rows, j] = null.reconstruction_errors - errors[rows]
        drawn = np.stack([[pair_draw(null.exposures[i], W, X[n].sum(), n, s, b, seed) for i, n in enumerate(rows)] for b in range(B)])
        flat = drawn.reshape(-1, V)
        f1 = solve(flat, W, np.tile(C[rows], (B, 1)), **kw).reconstruction_errors
        f0 = solve(flat, W, np.tile(C0, (B, 1)), **kw).reconstruction_errors
        null_statistics[:, rows, j] = (f0 - f1).reshape(B, rows.size)
    n_exceed, mean, p = reduce_null(statistic, null_statistics)
    return SimpleNamespace(statistic=statistic, p_value=p, n_exceed=n_exceed, tested=tested, exposures=exposures, reconstruction_errors=errors,
                           null_exposures=null_exposures, null_errors=null_errors, null_statistics=null_statistics, null_mean=mean)


def calibration_samples(seed=20240, share=0.2):
    """The samples of the calibration tests, host and device, built as ``_gof_ref.calibration_samples`` builds its own:
    (counts (72, 96), catalogue (5, 96), tested signature 4).  Rows 0..63 are multinomial draws of 2000 mutations from mixtures
    of the catalogue's first four signatures -- the tested one is absent; rows 64..71 the same with ``share`` of the mutations
    moved to the tested signature."""
    rng = np.random.default_rng(seed)
    V, K, T = 96, 4, 2000
    S = refit_ref.normalize(rng.dirichlet(np.full(V, 0.15), size=K + 1))
    E = rng.dirichlet(np.full(K, 1.0), size=72)
    spectra = E @ S[:K]
    spectra[64:] = (1.0 - share) * spectra[64:] + share * S[K]
    X = np.stack([rng.multinomial(T, p / p.sum()) for p in spectra]).astype(np.float64)
    return X, S, K
