"""Exposures to FIXED signatures under a negative-binomial likelihood, and the dispersion a cohort asks for
(``csrc/salnmf_nb.h``).

:func:`refit_exposures <salamander_amd.refit.refit_exposures>` models a sample's counts as Poisson around ``h W``.  Real
catalogues are overdispersed: the variance grows faster than the mean, and the Poisson refit lets the few largest channels of
a hypermutated sample dictate its exposures.  :func:`nb_refit_exposures` fits the negative-binomial model instead -- variance
``p + p**2 / alpha``, Poisson as ``alpha -> inf`` -- by the majorise-minimise step of the same shape (Gouvert et al. 2020;
Pelizzola et al. 2023), every sample iterated and stopped on its own, with a dispersion per sample.
:func:`estimate_dispersion` profiles the likelihood over a grid of ``alpha`` and says which value to pass, and whether the
negative binomial is needed at all.  There is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import time
from ctypes import c_double
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .refit import RefitResult, check_arguments, refit_exposures

EPSILON = float(np.finfo(np.float32).eps)
MAX_DISPERSION = 1e6  # towards infinity the second logarithm's argument is 1 to rounding; refit_exposures is the limit


@dataclass
class NBRefitResult(RefitResult):
    """:class:`RefitResult` with ``reconstruction_errors`` (and ``reconstruction_errors_resampled``) holding the
    negative-binomial divergence, plus the dispersions used and the samples' log-likelihoods."""

    dispersion: np.ndarray | None = None  # (N,)
    log_likelihood: np.ndarray | None = None  # (N,): -divergence + nb_constant(counts, dispersion)


@dataclass
class DispersionResult:
    grid: np.ndarray  # (A,)
    profile: np.ndarray  # (A, N): every sample's log-likelihood at every grid value
    dispersion: np.ndarray | float  # the grid value of largest cohort sum; (N,) each sample's own with per_sample
    at_upper_edge: np.ndarray | bool  # the argmax is the last grid value: Poisson is adequate at this resolution
    poisson_log_likelihood: np.ndarray  # (N,)
    lr_statistic: np.ndarray | float  # 2 (l_NB(dispersion) - l_Poisson), per cohort or per sample
    exposures: np.ndarray  # (A, N, K)
    divergence: np.ndarray  # (A, N)
    n_iterations: np.ndarray  # (A, N)
    converged: np.ndarray  # (A, N)
    timings: dict = field(default_factory=dict)


def check_dispersion(dispersion, n_samples: int) -> np.ndarray:
    """``dispersion`` as an ``(N,)`` float64 array, or ``ValueError``: a scalar or N values, finite, in (0, 1e6]."""
    try:
        a = np.asarray(dispersion, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("'dispersion' must be a number or an array of numbers.") from None
    if a.ndim == 0:
        a = np.full(n_samples, float(a))
    elif a.ndim != 1 or a.shape[0] != n_samples:
        raise ValueError(f"'dispersion' must be a scalar or hold one value per sample ({n_samples}), got shape {a.shape}.")
    if not np.isfinite(a).all():
        raise ValueError("'dispersion' must be finite: refit_exposures is the model at dispersion = inf.")
    if (a <= 0).any() or (a > MAX_DISPERSION).any():
        raise ValueError(f"'dispersion' must lie in (0, {MAX_DISPERSION:g}]: refit_exposures is the model beyond.")
    return np.ascontiguousarray(a)


def check_grid(grid) -> np.ndarray:
    """``grid`` as a float64 array, or ``ValueError``: at least one value, strictly increasing, each a valid dispersion."""
    try:
        g = np.asarray(grid, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("'grid' must be an array of numbers.") from None
    if g.ndim != 1 or g.size < 1:
        raise ValueError("'grid' must be a non-empty one-dimensional array.")
    g = check_dispersion(g, g.size)
    if (np.diff(g) <= 0).any():
        raise ValueError("'grid' must be strictly increasing.")
    return g


def nb_constant(counts, dispersion) -> np.ndarray:
    """The part of a row's negative-binomial log-likelihood that does not depend on the exposures, on the clipped counts:
    ``sum_v lgamma(x + a) - lgamma(a) - lgamma(x + 1) + x log x - (x + a) log(x + a) + a log a``, so that the row's
    log-likelihood is ``-divergence + nb_constant``."""
    from scipy.special import gammaln

    x = np.maximum(np.asarray(counts, dtype=np.float64), EPSILON)
    a = np.asarray(dispersion, dtype=np.float64).reshape(-1, 1)
    xa = x + a
    return (gammaln(xa) - gammaln(a) - gammaln(x + 1.0) + x * np.log(x) - xa * np.log(xa) + a * np.log(a)).sum(axis=1)


def poisson_constant(counts) -> np.ndarray:
    """``sum_v x log x - x - lgamma(x + 1)`` on the clipped counts: a row's Poisson log-likelihood is ``-KL + poisson_constant``."""
    from scipy.special import gammaln

    x = np.maximum(np.asarray(counts, dtype=np.float64), EPSILON)
    return (x * np.log(x) - x - gammaln(x + 1.0)).sum(axis=1)


def _call(X, S, alpha, R, seed, q, min_it, max_it, freq, tol, chunk, keep_resamples, device):
    (N, V), K = X.shape, S.shape[0]
    lib = _lib.load_with_device()
    Q = int(q.size)
    H = np.empty((N, K), dtype=np.float64)
    err = np.empty(N, dtype=np.float64)
    nit = np.empty(N, dtype=np.int32)
    conv = np.empty(N, dtype=np.int32)
    Hq = np.empty((Q, N, K), dtype=np.float64) if R else None
    Hm = np.empty((N, K), dtype=np.float64) if R else None
    nit_r = np.empty((R, N), dtype=np.int32) if R else None
    err_r = np.empty((R, N), dtype=np.float64) if R else None
    Hr = np.empty((R, N, K), dtype=np.float64) if R and keep_resamples else None
    ms = (c_double * 4)()
    p = _lib.pointer
    _lib.check(lib.salnmf_nb_refit_exposures(
        int(device), p(X), N, V, p(S), K, p(alpha), R, seed, Q if R else 0, p(q), min_it, max_it, freq, tol, chunk,
        p(H), p(err), p(nit), p(conv), p(Hq), p(Hm), p(nit_r), p(err_r), p(Hr), ctypes.cast(ms, _lib._D),
    ))
    return H, err, nit, conv, Hq, Hm, nit_r, err_r, Hr, ms


def nb_refit_exposures(counts, signatures, dispersion, n_resamples: int = 0, resample_seed: int = 0, quantiles=(0.025, 0.5, 0.975),
                       min_iterations: int = 500, max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7,
                       keep_resamples: bool = False, device: int = 0, chunk_bytes: int | None = None) -> NBRefitResult:
    """Negative-binomial exposures of every row of ``counts (N, V)`` to the fixed ``signatures (K, V)``, K <= 96 and V <= 96.

    ``dispersion`` is the negative binomial's ``alpha`` (variance ``p + p**2 / alpha``), a scalar or one value per sample,
    finite and in (0, 1e6]; :func:`estimate_dispersion` proposes one, and for ``alpha = inf`` call ``refit_exposures``.
    Everything else is ``refit_exposures``': the signature rows are divided by their sums and never clipped, every sample
    starts at ``h_k = sum(x) / K``, is iterated (``h_k <- h_k sum_v W_kv x_v / p_v / sum_v W_kv (x_v + alpha) / (p_v + alpha)``)
    and stopped on its own on its negative-binomial divergence ``sum_v x log(x / p) - (x + alpha) log((x + alpha) / (p + alpha))``
    (``reconstruction_errors``); ``n_resamples`` adds the bootstrap over ``resample_counts(counts, R, resample_seed)``, a
    resample of sample n carrying sample n's dispersion.  ``log_likelihood`` is ``-divergence + nb_constant(counts, dispersion)``.
    Anything out of range is a ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, S, R, seed, min_it, max_it, freq, tol, q, chunk = check_arguments(counts, signatures, n_resamples, resample_seed, quantiles, min_iterations,
                                                                         max_iterations, conv_test_freq, tol, chunk_bytes)
    alpha = check_dispersion(dispersion, X.shape[0])
    H, err, nit, conv, Hq, Hm, nit_r, err_r, Hr, ms = _call(X, S, alpha, R, seed, q, min_it, max_it, freq, tol, chunk, keep_resamples, device)
    timings = {"resample_s": ms[0] / 1e3, "refit_s": ms[1] / 1e3, "reduce_s": ms[2] / 1e3, "refit_kernel_ms": ms[1],
               "n_chunks": int(ms[3]), "total_s": time.perf_counter() - t_start}
    return NBRefitResult(exposures=H, reconstruction_errors=err, n_iterations=nit, converged=conv.astype(bool), exposures_quantiles=Hq,
                         exposures_mean=Hm, n_iterations_resampled=nit_r, reconstruction_errors_resampled=err_r, exposures_resampled=Hr,
                         quantiles=tuple(float(v) for v in q), timings=timings, dispersion=alpha, log_likelihood=-err + nb_constant(X, alpha))


def select_dispersion(grid, profile, poisson_log_likelihood, per_sample: bool = False):
    """``(dispersion, at_upper_edge, lr_statistic)`` of a profile ``(A, N)``: the first grid value of largest cohort sum (or of
    each sample's own column), whether it is the last one, and twice the log-likelihood gained over the Poisson fit."""
    grid, profile = np.asarray(grid, dtype=np.float64), np.asarray(profile, dtype=np.float64)
    if per_sample:
        best = np.argmax(profile, axis=0)
        top = profile[best, np.arange(profile.shape[1])]
        return grid[best], best == grid.size - 1, 2.0 * (top - poisson_log_likelihood)
    total = profile.sum(axis=1)
    best = int(np.argmax(total))
    return float(grid[best]), best == grid.size - 1, float(2.0 * (total[best] - np.sum(poisson_log_likelihood)))


def estimate_dispersion(counts, signatures, grid=np.geomspace(1, 1e4, 17), per_sample: bool = False, min_iterations: int = 500,
                        max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7, device: int = 0) -> DispersionResult:
    """The dispersion ``alpha`` of largest negative-binomial likelihood on a grid, for the cohort or per sample.

    Every sample is refitted at every grid value -- ``A x N`` problems in one list through one kernel launch, each carrying its
    own ``alpha`` -- and once under the Poisson model (``refit_exposures``).  ``profile[a, n]`` is sample n's log-likelihood at
    ``grid[a]``; ``dispersion`` the grid value whose cohort sum is largest (with ``per_sample`` each sample's own argmax, ``(N,)``);
    ``at_upper_edge`` says the argmax is the last grid value, i.e. Poisson is adequate at this resolution;
    ``poisson_log_likelihood = -KL + sum_v [x log x - x - lgamma(x + 1)]``; ``lr_statistic = 2 (l_NB(dispersion) - l_Poisson)``.
    ``grid`` must be strictly increasing with values in (0, 1e6].

    **No p-value is returned.**  ``alpha = inf`` lies on the boundary of the parameter space and the exposures are fitted too;
    calibrating ``lr_statistic`` needs draws from the fitted negative-binomial model (a gamma-Poisson generator on the device),
    which the library does not have yet.

    **Bias.**  With many free exposures the maximum-likelihood ``alpha`` is pushed upward: the exposures absorb part of the
    overdispersion.  Gamma-Poisson data drawn with ``alpha = 20``, N = 40, gave in a CPU prototype

    ====  ====  ==================================
    K     V     grid value chosen
    ====  ====  ==================================
    3     96    17.8 (a neighbour of the truth)
    17    33    56
    96    96    1e4 (top of the grid)
    ====  ====  ==================================

    so estimate on the candidate set you will fit with, not on the whole catalogue."""
    t_start = time.perf_counter()
    X, S, _, _, min_it, max_it, freq, tol, q, chunk = check_arguments(counts, signatures, 0, 0, (), min_iterations, max_iterations, conv_test_freq,
                                                                      tol, None)
    g = check_grid(grid)
    (N, V), K, A = X.shape, S.shape[0], g.size
    if A * N >= 2**31:
        raise ValueError(f"{A} grid values x {N} samples: at most 2**31 - 1 problems.")
    # problem (a, n) is row a N + n of the list: sample n at grid[a]
    H, err, nit, conv, *_, ms = _call(np.ascontiguousarray(np.tile(X, (A, 1))), S, np.repeat(g, N), 0, 0, q, min_it, max_it, freq, tol, chunk, False, device)
    divergence = err.reshape(A, N)
    profile = np.stack([-divergence[a] + nb_constant(X, np.full(N, g[a])) for a in range(A)])
    poisson = refit_exposures(X, S, min_iterations=min_it, max_iterations=max_it, conv_test_freq=freq, tol=tol, device=device)
    poisson_ll = -poisson.reconstruction_errors + poisson_constant(X)
    dispersion, edge, lr = select_dispersion(g, profile, poisson_ll, per_sample)
    timings = {"refit_s": ms[1] / 1e3, "refit_kernel_ms": ms[1], "poisson_refit_s": poisson.timings["refit_s"], "total_s": time.perf_counter() - t_start}
    return DispersionResult(grid=g, profile=profile, dispersion=dispersion, at_upper_edge=edge, poisson_log_likelihood=poisson_ll, lr_statistic=lr,
                            exposures=H.reshape(A, N, K), divergence=divergence, n_iterations=nit.reshape(A, N), converged=conv.reshape(A, N).astype(bool),
                            timings=timings)
