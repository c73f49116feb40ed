"""Exposures to FIXED signatures under a negative-binomial likelihood, and the dispersion a cohort asks for
(``csrc/salnmf_nb.h``).

:func:`refit_exposures <salamander_amd.refit.refit_exposures>` models a sample's counts as Poisson around ``h W``.  Real
catalogues are overdispersed: the variance grows faster than the mean, and the Poisson refit lets the few largest channels of
a hypermutated sample dictate its exposures.  :func:`nb_refit_exposures` fits the negative-binomial model instead -- variance
``p + p**2 / alpha``, Poisson as ``alpha -> inf`` -- by the majorise-minimise step of the same shape (Gouvert et al. 2020;
Pelizzola et al. 2023), every sample iterated and stopped on its own, with a dispersion per sample.
:func:`estimate_dispersion` profiles the likelihood over a grid of ``alpha`` and says which value to pass, and whether the
negative binomial is needed at all.  :func:`draw_nb_counts` draws count vectors from a fitted negative-binomial model on the
device (``csrc/salnmf_nbdraw.h``), :func:`nb_goodness_of_fit` is the parametric-bootstrap test of
:func:`goodness_of_fit <salamander_amd.gof.goodness_of_fit>` under that model, and :func:`dispersion_test` calibrates the
dispersion estimate: a p-value for ``lr_statistic`` and an interval for the estimate.  :func:`nb_assign_signatures` is
:func:`assign_signatures <salamander_amd.assign.assign_signatures>` under the negative-binomial model (``csrc/salnmf_nb_assign.h``,
DESIGN.md section 25): which signatures are active in each sample, with candidate sets, required signatures and the re-addition
pass.  :func:`nb_signature_presence_test` is
:func:`signature_presence_test <salamander_amd.presence.signature_presence_test>` under that model (``csrc/salnmf_nb_presence.h``,
DESIGN.md section 26): is signature s present in this sample, when the counts are overdispersed?  There is no CPU fallback.
"""

from __future__ import annotations

import time
from dataclasses import dataclass, field, fields

import numpy as np

from . import _lib
from .assign import AssignResult, assign_signatures, call_assign, check_sets, check_threshold
from .gof import GofResult, call_gof, check_integer_counts, check_model, check_n_draws, draw_model_counts
from .presence import PresenceResult, call_presence, check_presence_arguments
from .refit import RefitResult, call_refit, check_arguments, quantile_indices, refit_exposures
from .resample import check_seed

EPSILON = float(np.finfo(np.float32).eps)
MAX_DISPERSION = 1e6  # towards infinity the second logarithm's argument is 1 to rounding; refit_exposures is the limit
MAX_DRAW_MEAN = 2.0**24  # a model row's sum: the drawn total must stay far below 2**31


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
    fit = call_refit("salnmf_nb_refit_exposures", (alpha,), X, S, R, seed, q, min_it, max_it, freq, tol, chunk, keep_resamples, device, t_start)
    return NBRefitResult(**fit, dispersion=alpha, log_likelihood=-fit["reconstruction_errors"] + nb_constant(X, alpha))


@dataclass
class NBAssignResult(AssignResult):
    """:class:`AssignResult <salamander_amd.assign.AssignResult>` with ``reconstruction_errors``, ``dense_errors``, ``kl_increase``
    and ``kl_decrease`` holding negative-binomial divergences and their differences, plus the dispersions used and the samples'
    log-likelihoods at the sparse and at the phase-0 exposures."""

    dispersion: np.ndarray | None = None  # (N,)
    log_likelihood: np.ndarray | None = None  # (N,): -reconstruction_errors + nb_constant(counts, dispersion)
    dense_log_likelihood: np.ndarray | None = None  # (N,): -dense_errors + nb_constant(counts, dispersion)


def nb_assign_signatures(counts, signatures, dispersion, max_kl_increase: float = 1.92, n_resamples: int = 0, resample_seed: int = 0,
                         quantiles=(0.025, 0.5, 0.975), min_iterations: int = 500, max_iterations: int = 10000, conv_test_freq: int = 10,
                         tol: float = 1e-7, keep_resamples: bool = False, device: int = 0, chunk_bytes: int | None = None,
                         candidates=None, required=None, readd: bool = False) -> NBAssignResult:
    """Sparse negative-binomial exposures of every row of ``counts (N, V)`` to the fixed ``signatures (K, V)``, K <= 96 and V <= 96.

    :func:`assign_signatures <salamander_amd.assign.assign_signatures>` with the step and the divergence of
    :func:`nb_refit_exposures`: phase 0 on the candidate set (with no sets, ``nb_refit_exposures`` bit for bit), backward
    elimination of the active, unprotected signature of smallest exposure, and with ``readd=True`` the re-addition pass, all in
    one kernel launch.  ``dispersion`` is a scalar or one value per sample, in (0, 1e6]; a resample carries its sample's.  The
    difference of two negative-binomial divergences of one sample at one dispersion is a log-likelihood difference, so
    ``max_kl_increase = 1.92`` keeps its meaning: half the 95 % point of a chi-square with one degree of freedom.  The
    re-addition pass ranks the removed candidates by ``u_k = sum_v W_kv a_v / sum_v W_kv b_v`` at the accepted exposures
    (``a = x / p``, ``b = (x + alpha) / (p + alpha)``) and tries those with ``u_k > 1``.  ``candidates = required = A`` is the solve
    on the active set A: no trial, ``exposures == dense_exposures``, exactly 0.0 off A.  ``max_iterations`` must be a multiple
    of ``conv_test_freq``.  Anything out of range is a ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, S, R, seed, min_it, max_it, freq, tol, q, chunk = check_arguments(counts, signatures, n_resamples, resample_seed, quantiles, min_iterations,
                                                                         max_iterations, conv_test_freq, tol, chunk_bytes)
    alpha = check_dispersion(dispersion, X.shape[0])
    thr = check_threshold(max_it, freq, max_kl_increase)
    C, Rq, readd = check_sets(candidates, required, readd, X.shape[0], S.shape[0])
    fit = call_assign("salnmf_nb_assign_signatures", (alpha,), X, S, R, seed, q, min_it, max_it, freq, tol, thr, chunk, C, Rq, readd, keep_resamples,
                      device, t_start)
    const = nb_constant(X, alpha)
    return NBAssignResult(**fit, dispersion=alpha, log_likelihood=-fit["reconstruction_errors"] + const,
                          dense_log_likelihood=-fit["dense_errors"] + const)


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
                        max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7, device: int = 0,
                        candidates=None) -> DispersionResult:
    """The dispersion ``alpha`` of largest negative-binomial likelihood on a grid, for the cohort or per sample.

    Every sample is refitted at every grid value -- ``A x N`` problems in one list through one kernel launch, each carrying its
    own ``alpha`` -- and once under the Poisson model (``refit_exposures``).  ``profile[a, n]`` is sample n's log-likelihood at
    ``grid[a]``; ``dispersion`` the grid value whose cohort sum is largest (with ``per_sample`` each sample's own argmax, ``(N,)``);
    ``at_upper_edge`` says the argmax is the last grid value, i.e. Poisson is adequate at this resolution;
    ``poisson_log_likelihood = -KL + sum_v [x log x - x - lgamma(x + 1)]``; ``lr_statistic = 2 (l_NB(dispersion) - l_Poisson)``.
    ``grid`` must be strictly increasing with values in (0, 1e6].

    **No p-value is returned here.**  ``alpha = inf`` lies on the boundary of the parameter space and the exposures are fitted
    too, so ``lr_statistic`` has no textbook null law.  Its null is the Poisson model, though, whose draws
    (``draw_model_counts``) the library has: :func:`dispersion_test` drives this estimate over them and returns the p-value.

    **Bias.**  With many free exposures the maximum-likelihood ``alpha`` is pushed upward: the exposures absorb part of the
    overdispersion.  Gamma-Poisson data drawn with ``alpha = 20``, N = 40, gave in a CPU prototype

    ====  ====  ==================================
    K     V     grid value chosen
    ====  ====  ==================================
    3     96    17.8 (a neighbour of the truth)
    17    33    56
    96    96    1e4 (top of the grid)
    ====  ====  ==================================

    so estimate on the candidate set you will fit with, not on the whole catalogue: ``candidates`` is ``None`` or a boolean mask of
    shape (K,) or (N, K), the signatures each sample may use.  With a mask every one of the ``A x N`` problems is solved on its
    sample's set (:func:`nb_assign_signatures` with ``candidates = required =`` the mask: one solve, no trial), the Poisson fit is
    ``assign_signatures(candidates=mask, required=mask)``, ``exposures`` are exactly 0.0 off the set, and ``max_iterations`` must be
    a multiple of ``conv_test_freq``.  With ``None`` the call is what it was, bit for bit."""
    t_start = time.perf_counter()
    X, S, _, _, min_it, max_it, freq, tol, q, chunk = check_arguments(counts, signatures, 0, 0, (), min_iterations, max_iterations, conv_test_freq,
                                                                      tol, None)
    g = check_grid(grid)
    (N, V), K, A = X.shape, S.shape[0], g.size
    if A * N >= 2**31:
        raise ValueError(f"{A} grid values x {N} samples: at most 2**31 - 1 problems.")
    if candidates is not None:
        return _estimate_on_sets(X, S, g, per_sample, min_it, max_it, freq, tol, q, chunk, device, candidates, t_start)
    # problem (a, n) is row a N + n of the list: sample n at grid[a]
    fit = call_refit("salnmf_nb_refit_exposures", (np.repeat(g, N),), np.ascontiguousarray(np.tile(X, (A, 1))), S, 0, 0, q, min_it, max_it, freq, tol,
                     chunk, False, device)
    H, nit, conv, ms = fit["exposures"], fit["n_iterations"], fit["converged"], fit["timings"]["refit_kernel_ms"]
    divergence = fit["reconstruction_errors"].reshape(A, N)
    profile = np.stack([-divergence[a] + nb_constant(X, np.full(N, g[a])) for a in range(A)])
    poisson = refit_exposures(X, S, min_iterations=min_it, max_iterations=max_it, conv_test_freq=freq, tol=tol, device=device)
    poisson_ll = -poisson.reconstruction_errors + poisson_constant(X)
    dispersion, edge, lr = select_dispersion(g, profile, poisson_ll, per_sample)
    timings = {"refit_s": ms / 1e3, "refit_kernel_ms": ms, "poisson_refit_s": poisson.timings["refit_s"], "total_s": time.perf_counter() - t_start}
    return DispersionResult(grid=g, profile=profile, dispersion=dispersion, at_upper_edge=edge, poisson_log_likelihood=poisson_ll, lr_statistic=lr,
                            exposures=H.reshape(A, N, K), divergence=divergence, n_iterations=nit.reshape(A, N), converged=conv.reshape(A, N),
                            timings=timings)


def _estimate_on_sets(X, S, g, per_sample, min_it, max_it, freq, tol, q, chunk, device, candidates, t_start) -> DispersionResult:
    """:func:`estimate_dispersion` with a candidate mask: the same problem list, every problem solved on its sample's set."""
    (N, V), K, A = X.shape, S.shape[0], g.size
    thr = check_threshold(max_it, freq, 0.0)
    C, _, _ = check_sets(candidates, None, False, N, K)
    tiled = np.ascontiguousarray(np.tile(C, (A, 1)))  # problem (a, n) is row a N + n: sample n at grid[a], on C_n
    fit = call_assign("salnmf_nb_assign_signatures", (np.repeat(g, N),), np.ascontiguousarray(np.tile(X, (A, 1))), S, 0, 0, q, min_it, max_it, freq,
                      tol, thr, chunk, tiled, tiled, False, False, device, time.perf_counter())
    ms = fit["timings"]["assign_kernel_ms"]
    divergence = fit["reconstruction_errors"].reshape(A, N)
    profile = np.stack([-divergence[a] + nb_constant(X, np.full(N, g[a])) for a in range(A)])
    poisson = assign_signatures(X, S, min_iterations=min_it, max_iterations=max_it, conv_test_freq=freq, tol=tol, device=device, candidates=C,
                                required=C)
    poisson_ll = -poisson.reconstruction_errors + poisson_constant(X)
    dispersion, edge, lr = select_dispersion(g, profile, poisson_ll, per_sample)
    timings = {"refit_s": ms / 1e3, "refit_kernel_ms": ms, "poisson_refit_s": poisson.timings["assign_s"], "total_s": time.perf_counter() - t_start}
    return DispersionResult(grid=g, profile=profile, dispersion=dispersion, at_upper_edge=edge, poisson_log_likelihood=poisson_ll, lr_statistic=lr,
                            exposures=fit["exposures"].reshape(A, N, K), divergence=divergence,
                            n_iterations=fit["n_iterations"].astype(np.int32).reshape(A, N), converged=fit["converged"].reshape(A, N), timings=timings)


@dataclass
class NBGofResult(GofResult):
    """:class:`GofResult <salamander_amd.gof.GofResult>` of the negative-binomial model: ``exposures`` as ``nb_refit_exposures``
    returns them, ``reconstruction_errors`` and ``null_errors`` the negative-binomial divergences, plus the dispersions used and
    the samples' log-likelihoods."""

    dispersion: np.ndarray | None = None  # (N,)
    log_likelihood: np.ndarray | None = None  # (N,): -divergence + nb_constant(counts, dispersion)


@dataclass
class DispersionTestResult:
    estimate: DispersionResult  # estimate_dispersion of the counts
    dispersion: np.ndarray | float  # = estimate.dispersion
    at_upper_edge: np.ndarray | bool
    lr_statistic: np.ndarray | float
    p_value: np.ndarray | float  # (1 + #{null_lr >= lr_statistic}) / (B + 1) under the Poisson null
    null_lr: np.ndarray  # (B,), or (B, N) with per_sample
    dispersion_draws: np.ndarray | None = None  # (B,), or (B, N): the estimate on cohorts drawn from the NB fit at `dispersion`
    dispersion_interval: np.ndarray | None = None  # (Q,) or (Q, N): order statistics of dispersion_draws, taken outward
    dispersion_bias: np.ndarray | float | None = None  # median(dispersion_draws) / dispersion
    quantiles: tuple = ()
    timings: dict = field(default_factory=dict)


def _failed_rows(n_failed: int, what: str) -> None:
    if n_failed:
        raise RuntimeError(f"salnmf: {what}: {n_failed} drawn rows ran out of attempts or reached a total of 2**31 and were written as zeros.")


def draw_nb_counts(exposures, signatures, dispersion, n_draws: int, seed: int = 0, device: int = 0) -> np.ndarray:
    """``n_draws`` count matrices drawn from the negative-binomial model around ``exposures (N, K) @ signatures (K, V)``:
    ``(n_draws, N, V)`` float64 of integer values, entry (n, v) of every draw a gamma-Poisson count of mean ``P[n, v]`` and
    variance ``P + P**2 / dispersion[n]`` (the contract: DESIGN.md section 24).  The draw is unconditional -- row totals
    vary, unlike ``draw_model_counts`` -- because the negative-binomial refit leaves the scale free.  The signature rows are
    divided by their sums; the exposures are finite and non-negative with row sums of at most 2**24; ``dispersion`` is a scalar
    or one value per row, in (0, 1e6].  The same bits on every run, and draw b does not depend on ``n_draws``."""
    H, S = check_model(exposures, signatures)
    (N, K), V = H.shape, S.shape[1]
    alpha = check_dispersion(dispersion, N)
    rows = np.flatnonzero(~((H @ S).sum(axis=1) <= MAX_DRAW_MEAN))
    if rows.size:
        raise ValueError(f"draw_nb_counts needs model row sums of at most 2**24: row {int(rows[0])} sums to {(H[int(rows[0])] @ S).sum():g}.")
    B, seed = check_n_draws(n_draws), check_seed(seed)
    lib = _lib.load_with_device()
    out = np.empty((B, N, V), dtype=np.float64)
    failed = np.zeros(1, dtype=np.int32)
    p = _lib.pointer
    _lib.check(lib.salnmf_draw_nb_counts(int(device), p(H), N, K, p(S), V, p(alpha), B, seed, p(out), p(failed)))
    _failed_rows(int(failed[0]), "draw_nb_counts")
    return out


def nb_goodness_of_fit(counts, signatures, dispersion, n_draws: int = 200, seed: int = 0, keep_draws: bool = False, min_iterations: int = 500,
                       max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7, chunk_bytes: int | None = None,
                       device: int = 0) -> NBGofResult:
    """The parametric-bootstrap test of every row of ``counts (N, V)`` against the fixed ``signatures (K, V)`` under the
    negative-binomial model with ``dispersion`` (a scalar or one value per sample, in (0, 1e6]).

    The observed fit is ``nb_refit_exposures(counts, signatures, dispersion, ...)`` bit for bit.  Draw b is
    ``draw_nb_counts(exposures, signatures, dispersion, n_draws, seed)[b]`` and its refit
    ``nb_refit_exposures(draws[b], signatures, dispersion, ...)``, bit for bit, with the same iteration arguments: the data and
    the null go through one procedure.  ``p_value`` is ``(1 + n_exceed) / (n_draws + 1)``: small where the catalogue does not
    explain the sample even with the variance ``p + p**2 / dispersion``.  Unlike ``goodness_of_fit`` the null vectors are not
    conditional on the sample's total: the negative-binomial refit leaves the scale free, and the model's law of the total is
    part of what is tested.  The counts are non-negative integers with row totals of at most 2**24; anything out of range is a
    ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, S, _, seed, min_it, max_it, freq, tol, _, chunk = check_arguments(counts, signatures, 0, seed, (), min_iterations, max_iterations,
                                                                        conv_test_freq, tol, chunk_bytes)
    check_integer_counts(X)
    rows = np.flatnonzero(X.sum(axis=1) > MAX_DRAW_MEAN)
    if rows.size:
        raise ValueError(f"nb_goodness_of_fit needs row totals of at most 2**24: row {int(rows[0])} sums to {X[int(rows[0])].sum():.0f}.")
    alpha = check_dispersion(dispersion, X.shape[0])
    B = check_n_draws(n_draws)
    fields, failed = call_gof("salnmf_nb_goodness_of_fit", (alpha,), X, S, B, seed, min_it, max_it, freq, tol, chunk, keep_draws, device, t_start,
                              count_failed=True)
    _failed_rows(failed, "nb_goodness_of_fit")
    return NBGofResult(**fields, dispersion=alpha, log_likelihood=-fields["reconstruction_errors"] + nb_constant(X, alpha))


@dataclass
class NBPresenceResult(PresenceResult):
    """:class:`PresenceResult <salamander_amd.presence.PresenceResult>` of the negative-binomial model: ``reconstruction_errors``,
    ``null_errors`` and the statistics are negative-binomial divergences and their differences, plus the dispersions used and the
    log-likelihoods of the two fits."""

    dispersion: np.ndarray | None = None  # (N,)
    log_likelihood: np.ndarray | None = None  # (N,): the alternative's, -reconstruction_errors + nb_constant(counts, dispersion)
    null_log_likelihood: np.ndarray | None = None  # (N, S): -null_errors + nb_constant(counts, dispersion)


def nb_signature_presence_test(counts, signatures, dispersion, test, n_draws: int = 200, seed: int = 0, candidates=None, keep_draws: bool = False,
                               min_iterations: int = 500, max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7,
                               chunk_bytes: int | None = None, device: int = 0) -> NBPresenceResult:
    """The bootstrap likelihood-ratio test of every signature in ``test`` in every row of ``counts (N, V)`` against the fixed
    ``signatures (K, V)`` under the negative-binomial model with ``dispersion`` (a scalar or one value per sample, in (0, 1e6]).

    :func:`signature_presence_test <salamander_amd.presence.signature_presence_test>` with the step and the divergence of
    :func:`nb_refit_exposures` and the draw of :func:`draw_nb_counts`.  With C the sample's candidate set and s = ``test[j]``: the
    alternative is ``nb_assign_signatures(x, signatures, dispersion, candidates=C, required=C, ...)`` and the null the same call on
    C without s, bit for bit; ``statistic[n, j] = f0 - f1`` is a difference of two negative-binomial divergences at one dispersion,
    a log-likelihood difference.  Null draw b is a gamma-Poisson draw from the fit without s with the sample's dispersion and goes
    through the same two solves.  Unlike the Poisson test the null vectors are **not conditional on the sample's total**: the
    negative-binomial refit leaves the scale free, and null totals vary as in :func:`nb_goodness_of_fit`.  On overdispersed counts
    the Poisson test's null is too tight and it rejects too often; this one's null carries the variance ``p + p**2 / dispersion``.
    Untested pairs, ``p_value``, ``max_iterations`` and ``chunk_bytes`` as in the Poisson test.  The counts are non-negative
    integers; a null fit whose mean total exceeds 2**24 is a ``RuntimeError`` from the library; everything else out of range is a
    ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, W, T, C, B, seed, min_it, max_it, freq, tol, chunk = check_presence_arguments(counts, signatures, test, n_draws, seed, candidates, min_iterations,
                                                                                     max_iterations, conv_test_freq, tol, chunk_bytes)
    alpha = check_dispersion(dispersion, X.shape[0])
    out, ms, failed = call_presence("salnmf_nb_signature_presence", (alpha,), X, W, T, C, B, seed, min_it, max_it, freq, tol, chunk, keep_draws, device,
                                    count_failed=True)
    _failed_rows(failed, "nb_signature_presence_test")
    res = out.result(T, C, ms, time.perf_counter() - t_start)
    const = nb_constant(X, alpha)
    return NBPresenceResult(**{f.name: getattr(res, f.name) for f in fields(res)}, dispersion=alpha, log_likelihood=-res.reconstruction_errors + const,
                            null_log_likelihood=-res.null_errors + const[:, None])


def _cohort_profiles(cohorts, S, g, poisson: bool, it, device):
    """``(profile (C, A, N), poisson log-likelihood (C, N) or None)`` of C cohorts ``(C, N, V)``: every cohort's A x N problem list,
    one after the other, in ONE negative-binomial launch, and one Poisson refit of the C N rows."""
    C, N, V = cohorts.shape
    A = g.size
    rows = np.ascontiguousarray(np.tile(cohorts[:, None], (1, A, 1, 1)).reshape(C * A * N, V))  # problem (c, a, n): sample n of cohort c at grid[a]
    fit = call_refit("salnmf_nb_refit_exposures", (np.tile(np.repeat(g, N), C),), rows, S, 0, 0, np.empty(0), *it, 0, False, device)
    divergence = fit["reconstruction_errors"].reshape(C, A, N)
    profile = np.stack([[-divergence[c, a] + nb_constant(cohorts[c], np.full(N, g[a])) for a in range(A)] for c in range(C)])
    if not poisson:
        return profile, None
    flat = np.ascontiguousarray(cohorts.reshape(C * N, V))
    fit = refit_exposures(flat, S, min_iterations=it[0], max_iterations=it[1], conv_test_freq=it[2], tol=it[3], device=device)
    return profile, (-fit.reconstruction_errors + poisson_constant(flat)).reshape(C, N)


def dispersion_test(counts, signatures, grid=np.geomspace(1, 1e4, 17), n_draws: int = 200, seed: int = 0, interval: bool = True,
                    quantiles=(0.025, 0.5, 0.975), per_sample: bool = False, min_iterations: int = 500, max_iterations: int = 10000,
                    conv_test_freq: int = 10, tol: float = 1e-7, chunk_bytes: int | None = None, device: int = 0) -> DispersionTestResult:
    """:func:`estimate_dispersion` with its two calibrations: is ``lr_statistic`` large, and how sure and how biased is the estimate?

    **p_value.**  The null of ``lr_statistic`` is ``alpha = inf``, the Poisson model.  ``n_draws`` cohorts are drawn from the
    Poisson fit (``draw_model_counts`` of ``refit_exposures``' exposures and the samples' totals), each goes through the same
    A x N problem list and one Poisson refit, and ``p_value = (1 + #{null_lr >= lr_statistic}) / (n_draws + 1)``, for the cohort
    or, with ``per_sample``, per sample.  The procedure applied to the data is applied to the null, so the boundary and the
    fitted exposures are accounted for, and so is the negative ``lr_statistic`` that a finite top of the grid gives on Poisson data.

    **dispersion_draws, dispersion_interval, dispersion_bias** (``interval=True``).  ``n_draws`` cohorts are drawn from the
    negative-binomial fit at the estimate (``draw_nb_counts`` of the exposures fitted at ``dispersion``) and each is re-estimated on
    the grid.  ``dispersion_interval`` holds the order statistics of those estimates at ``quantiles``, taken outward;
    ``dispersion_bias = median(dispersion_draws) / dispersion``.  With many free exposures the maximum-likelihood ``alpha`` is
    pushed upward (the exposures absorb part of the overdispersion; data drawn with ``alpha = 20``, N = 40, gave 17.8 at K = 3,
    56 at (K, V) = (17, 33) and the top of the grid at K = 96): a bias well above 1 is that effect at your K, and the interval is
    one of the biased estimator around the estimate, not a corrected one.

    **Both statements are conditional on the grid.**  The estimate and every re-estimate are grid values; an estimate at the last
    grid value (``at_upper_edge``) says "Poisson is adequate at this resolution", its draws mostly sit at the edge too, and the
    interval then only says so.  The p-value is that of the statistic computed on this grid.

    Draws are processed in chunks whose tiled problem list stays within ``chunk_bytes`` (default 256 MiB).  Anything out of range
    is a ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, S, _, seed, min_it, max_it, freq, tol, q, chunk = check_arguments(counts, signatures, 0, seed, quantiles, min_iterations, max_iterations,
                                                                        conv_test_freq, tol, chunk_bytes)
    check_integer_counts(X)
    g = check_grid(grid)
    B = check_n_draws(n_draws)
    if not isinstance(interval, (bool, np.bool_)) or not isinstance(per_sample, (bool, np.bool_)):
        raise ValueError("'interval' and 'per_sample' must be booleans.")
    (N, V), A = X.shape, g.size
    if A * N >= 2**31:
        raise ValueError(f"{A} grid values x {N} samples: at most 2**31 - 1 problems.")
    if interval and (X.sum(axis=1) > MAX_DRAW_MEAN).any():
        raise ValueError("dispersion_test(interval=True) needs row totals of at most 2**24.")
    it = (min_it, max_it, freq, tol)
    kw = dict(min_iterations=min_it, max_iterations=max_it, conv_test_freq=freq, tol=tol, device=device)
    est = estimate_dispersion(X, S, g, per_sample=per_sample, **kw)
    # cohorts per chunk: the tiled [A N][V] lists of a chunk stay within chunk_bytes (at least one cohort)
    per_chunk = int(max(1, min(B, (chunk if chunk > 0 else 256 << 20) // (8 * A * N * V), (2**31 - 1) // (A * N))))

    def estimates(cohorts, poisson):
        out_alpha, out_lr = [], []
        for first in range(0, B, per_chunk):
            part = cohorts[first:first + per_chunk]
            profile, pois = _cohort_profiles(part, S, g, poisson, it, device)
            for c in range(part.shape[0]):
                a, _, lr = select_dispersion(g, profile[c], pois[c] if poisson else np.zeros(N), per_sample)
                out_alpha.append(a), out_lr.append(lr)
        return np.array(out_alpha), np.array(out_lr)

    fit0 = refit_exposures(X, S, **kw)
    _, null_lr = estimates(draw_model_counts(fit0.exposures, S, X.sum(axis=1), B, seed, device=device), True)
    p_value = (1 + (null_lr >= est.lr_statistic).sum(axis=0)) / (B + 1)
    res = DispersionTestResult(estimate=est, dispersion=est.dispersion, at_upper_edge=est.at_upper_edge, lr_statistic=est.lr_statistic,
                               p_value=p_value if per_sample else float(p_value), null_lr=null_lr, quantiles=tuple(float(v) for v in q))
    if interval:
        best = np.searchsorted(g, np.broadcast_to(est.dispersion, (N,)))
        H = est.exposures[best, np.arange(N)]  # every sample's exposures at the estimate
        draws, _ = estimates(draw_nb_counts(H, S, est.dispersion, B, seed, device=device), False)
        order = np.sort(draws, axis=0)
        res.dispersion_draws, res.dispersion_interval = draws, order[quantile_indices(q, B)]
        res.dispersion_bias = np.median(draws, axis=0) / est.dispersion
        if not per_sample:
            res.dispersion_bias = float(res.dispersion_bias)
    res.timings = {"total_s": time.perf_counter() - t_start, "cohorts_per_chunk": per_chunk}
    return res
