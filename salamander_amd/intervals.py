"""How far can one exposure move before the sample's fit degrades?  The profile likelihood of an exposure and the confidence
interval it gives, per (sample, tested signature) (``csrc/salnmf_profile.h``).

The bootstrap percentiles of :func:`refit_exposures` are intervals of a dense refit in which no exposure is ever zero: for an
absent signature they never contain 0, and they are not tied to the threshold on which :func:`assign_signatures` removes a
signature.  The profile-likelihood interval is: all values c for which fixing ``h_s = c`` and re-solving the sample's other
exposures raises its KL divergence by at most ``max_kl_increase`` over the fit on the whole candidate set.  It needs no random
numbers, and its lower end is exactly 0 precisely when removing s costs at most ``max_kl_increase`` -- the criterion of
:func:`assign_signatures` and the statistic of :func:`signature_presence_test`.  :func:`profile_likelihood` evaluates the
profile on given values, :func:`exposure_intervals` searches its two ends.  Everything runs on the device; there is no CPU
fallback.
"""

from __future__ import annotations

import ctypes
import time
from ctypes import c_double
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .assign import check_sets
from .presence import check_test
from .refit import check_arguments

MAX_VALUES = 4096  # salnmf_profile.h: PROFILE_MAX_VALUES
MAX_BISECTIONS = 64  # PROFILE_MAX_BISECTIONS
MAX_EXPANSIONS = 1000  # PROFILE_MAX_EXPANSIONS


@dataclass
class ProfileResult:
    profile: np.ndarray  # (N, S, M): g(c) = f(c) - f1; NaN where the pair is untested
    errors: np.ndarray  # (N, S, M): f(c), the sample's KL divergence after the solve with h_s frozen at c
    n_iterations: np.ndarray  # (N, S, M) int32
    converged: np.ndarray  # (N, S, M) bool
    values: np.ndarray  # (M,) or (N, S, M) as given
    exposures: np.ndarray  # (N, K): the alternative fit, on the candidate set (NaN rows where no pair of the sample is tested)
    reconstruction_errors: np.ndarray  # (N,): f1
    tested: np.ndarray  # (N, S) bool: s is a candidate of the sample and not its only one
    test: tuple = ()
    candidates: np.ndarray | None = None  # (N, K) bool as applied, None = every signature
    profile_exposures: np.ndarray | None = None  # (N, S, M, K) with keep_exposures: entry s exactly c, exactly 0.0 off the set
    timings: dict = field(default_factory=dict)


@dataclass
class IntervalResult:
    lower: np.ndarray  # (N, S): exactly 0.0 where statistic <= max_kl_increase, above 0 elsewhere; NaN where the pair is untested
    upper: np.ndarray  # (N, S): +inf where the expansion found no bracket
    estimate: np.ndarray  # (N, S): exposures[n, s]
    bracketed: np.ndarray  # (N, S) bool: the upper end was bracketed
    n_trials: np.ndarray  # (N, S, 2) int32: frozen solves spent on the lower and on the upper end
    statistic: np.ndarray  # (N, S): g(0) = f0 - f1, signature_presence_test's statistic
    null_errors: np.ndarray  # (N, S): f0
    exposures: np.ndarray  # (N, K): the alternative fit
    reconstruction_errors: np.ndarray  # (N,): f1
    tested: np.ndarray  # (N, S) bool
    max_kl_increase: float = 1.92
    test: tuple = ()
    candidates: np.ndarray | None = None
    trace_values: np.ndarray | None = None  # (N, S, 2, max_expansions + n_bisections) with keep_trace: the trials in order, NaN past n_trials
    trace_profile: np.ndarray | None = None  # the same shape: g at every trial
    timings: dict = field(default_factory=dict)


def _integer(value, lo: int, hi: int, name: str) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"'{name}' must be an integer in [{lo}, {hi}].")
    return int(value)


def check_profile_arguments(counts, signatures, test, candidates, min_iterations, max_iterations, conv_test_freq, tol):
    """What both calls check of their shared arguments before they touch a device -> ``(X, W, T, C, min_it, max_it, freq, tol)``:
    everything :func:`signature_presence_test` refuses of them, except counts that are not integers."""
    X, W, _, _, min_it, max_it, freq, tol, _, _ = check_arguments(counts, signatures, 0, 0, (), min_iterations, max_iterations, conv_test_freq, tol, None)
    if max_it % freq != 0:
        raise ValueError("'max_iterations' must be a multiple of 'conv_test_freq': the solves of a pair follow one another on the device.")
    T = check_test(test, W.shape[0])
    C, _, _ = check_sets(candidates, None, False, X.shape[0], W.shape[0])
    return X, W, T, C, min_it, max_it, freq, tol


def check_values(values, N: int, S: int) -> np.ndarray:
    """``values`` as a contiguous float64 array of shape (M,) or (N, S, M), 1 <= M <= 4096, finite and not negative."""
    message = f"'values' must hold finite numbers >= 0 in shape (M,) or ({N}, {S}, M) with 1 <= M <= {MAX_VALUES}."
    if isinstance(values, (str, bytes)) or values is None:
        raise ValueError(message)
    try:
        raw = np.asarray(values)
    except (TypeError, ValueError):
        raise ValueError(message) from None
    if raw.dtype == bool or not (np.issubdtype(raw.dtype, np.integer) or np.issubdtype(raw.dtype, np.floating)):
        raise ValueError(message)
    out = np.ascontiguousarray(raw, dtype=np.float64)
    if not (out.ndim == 1 or (out.ndim == 3 and out.shape[:2] == (N, S))) or not 1 <= out.shape[-1] <= MAX_VALUES:
        raise ValueError(message)
    if not np.isfinite(out).all() or (out < 0.0).any():
        raise ValueError(message)
    return out


def _mask_bytes(C):
    return None if C is None else np.ascontiguousarray(C, dtype=np.uint8)


def profile_likelihood(counts, signatures, test, values, candidates=None, min_iterations: int = 500, max_iterations: int = 10000,
                       conv_test_freq: int = 10, tol: float = 1e-7, keep_exposures: bool = False, device: int = 0) -> ProfileResult:
    """The profile of the sample's KL divergence along one exposure, for every signature in ``test`` and every row of
    ``counts (N, V)`` against the fixed ``signatures (K, V)``, K <= 96 and V <= 96.

    With C the sample's candidate set (``candidates`` as :func:`signature_presence_test` takes it), s = ``test[j]`` and c a value:
    the frozen solve starts from ``h_s = c``, ``h_k = sum(x) / (|C| - 1)`` on C without s and exactly 0.0 off C, applies the
    refit's update to the members of C other than s and never touches ``h_s``; ``errors[n, j, i] = f(c)`` is the divergence it
    ends at under the refit's stop rule, and ``profile[n, j, i] = f(c) - f1`` with f1 the fit on C (``reconstruction_errors``).
    At ``c = 0.0`` the solve is bit for bit :func:`signature_presence_test`'s null solve and the profile its ``statistic``.
    ``values`` has shape (M,) -- the same for every pair -- or (N, S, M); every value is finite and >= 0.  A pair with s outside
    C or C = {s} is untested: NaN, ``tested`` False, no solve.  The counts need not be integers.  ``max_iterations`` must be a
    multiple of ``conv_test_freq``.  Anything out of range is a ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, W, T, C, min_it, max_it, freq, tol = check_profile_arguments(counts, signatures, test, candidates, min_iterations, max_iterations,
                                                                    conv_test_freq, tol)
    (N, V), K, S = X.shape, W.shape[0], int(T.size)
    vals = check_values(values, N, S)
    M = int(vals.shape[-1])
    lib = _lib.load_with_device()
    tested = np.zeros((N, S), dtype=np.uint8)
    # (the library fills every entry; an untested pair's are NaN and 0)
    profile, errors = np.full((N, S, M), np.nan), np.full((N, S, M), np.nan)
    nit, conv = np.zeros((N, S, M), dtype=np.int32), np.zeros((N, S, M), dtype=np.int32)
    Hc = np.full((N, S, M, K), np.nan) if keep_exposures else None
    H, err = np.full((N, K), np.nan), np.full(N, np.nan)
    ms = (c_double * 3)()
    p = _lib.pointer
    _lib.check(lib.salnmf_profile_likelihood(
        int(device), p(X), N, V, p(W), K, p(T), S, p(_mask_bytes(C)), p(vals), M, int(vals.ndim == 3), min_it, max_it, freq, tol, p(tested), p(profile),
        p(errors), p(nit), p(conv), p(Hc), p(H), p(err), ctypes.cast(ms, _lib._D),
    ))
    timings = {"observed_kernel_ms": ms[0], "profile_kernel_ms": ms[1], "n_problems": int(ms[2]), "total_s": time.perf_counter() - t_start}
    return ProfileResult(profile=profile, errors=errors, n_iterations=nit, converged=conv.astype(bool), values=vals, exposures=H,
                         reconstruction_errors=err, tested=tested.astype(bool), test=tuple(int(v) for v in T), candidates=C, profile_exposures=Hc,
                         timings=timings)


def exposure_intervals(counts, signatures, test, candidates=None, max_kl_increase: float = 1.92, n_bisections: int = 16, max_expansions: int = 40,
                       keep_trace: bool = False, min_iterations: int = 500, max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7,
                       device: int = 0) -> IntervalResult:
    """The profile-likelihood interval of the exposure to every signature in ``test``, in every row of ``counts (N, V)``: all c
    with ``profile(c) <= max_kl_increase`` (:func:`profile_likelihood`), its two ends searched on the device.

    ``max_kl_increase`` is half a chi-square quantile with one degree of freedom: the default 1.92 is half the 95 % point 3.84,
    the threshold :func:`assign_signatures` removes a signature on; for another level take
    ``0.5 * scipy.stats.chi2.ppf(level, 1)`` (1.35 for 90 %, 3.32 for 99 %).  With ``estimate = exposures[n, s]`` and
    ``statistic = profile(0)``:

    lower end: ``statistic <= max_kl_increase`` gives exactly 0.0 without a trial -- removing s costs no more than the threshold.
    Otherwise ``lo = 0, hi = estimate`` and ``n_bisections`` halvings; while ``lo`` is still 0 after them (the end lies below
    ``estimate / 2**n_bisections``) the halving goes on, at most ``max_expansions`` more times, up to the first trial outside;
    ``lower = lo``.  So a lower end of 0 says the same as ``statistic <= max_kl_increase``.
    upper end: trials at ``estimate + d * 2**e`` with ``d = max(estimate, 1.0)``, e = 0, 1, ..., until the profile exceeds the
    threshold; without a bracket after ``max_expansions`` trials ``upper = inf`` and ``bracketed`` is False.  Otherwise
    ``n_bisections`` halvings; ``upper = hi``.

    Both ends are the outer ends of their last bracket, so the returned interval contains the exact one and is at most
    ``bracket / 2**n_bisections`` wider at each end.  A comparison with a NaN counts as false.  ``keep_trace`` returns every
    trial value and its profile.  The intervals are per sample and per signature, conditional on the catalogue, and not
    corrected for multiplicity; an untested pair (s outside the set, or alone in it) has NaN ends.  The remaining arguments
    are :func:`profile_likelihood`'s; anything out of range is a ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, W, T, C, min_it, max_it, freq, tol = check_profile_arguments(counts, signatures, test, candidates, min_iterations, max_iterations,
                                                                    conv_test_freq, tol)
    if isinstance(max_kl_increase, (bool, np.bool_, str)) or not isinstance(max_kl_increase, (int, float, np.integer, np.floating)) \
            or not np.isfinite(max_kl_increase) or max_kl_increase < 0:
        raise ValueError("'max_kl_increase' must be a finite number >= 0.")
    delta = float(max_kl_increase)
    J = _integer(n_bisections, 0, MAX_BISECTIONS, "n_bisections")
    E = _integer(max_expansions, 1, MAX_EXPANSIONS, "max_expansions")
    (N, V), K, S = X.shape, W.shape[0], int(T.size)
    lib = _lib.load_with_device()
    tested, bracketed = np.zeros((N, S), dtype=np.uint8), np.zeros((N, S), dtype=np.uint8)
    # (the library fills every entry; an untested pair's are NaN and 0)
    lower, upper, estimate, stat, err0 = (np.full((N, S), np.nan) for _ in range(5))
    n_trials = np.zeros((N, S, 2), dtype=np.int32)
    H, err = np.full((N, K), np.nan), np.full(N, np.nan)
    trace_c = np.full((N, S, 2, E + J), np.nan) if keep_trace else None
    trace_g = np.full((N, S, 2, E + J), np.nan) if keep_trace else None
    ms = (c_double * 3)()
    p = _lib.pointer
    _lib.check(lib.salnmf_exposure_intervals(
        int(device), p(X), N, V, p(W), K, p(T), S, p(_mask_bytes(C)), delta, J, E, min_it, max_it, freq, tol, p(tested), p(lower), p(upper), p(estimate),
        p(bracketed), p(n_trials), p(stat), p(err0), p(H), p(err), p(trace_c), p(trace_g), ctypes.cast(ms, _lib._D),
    ))
    timings = {"observed_kernel_ms": ms[0], "profile_kernel_ms": ms[1], "n_problems": int(ms[2]), "total_s": time.perf_counter() - t_start}
    return IntervalResult(lower=lower, upper=upper, estimate=estimate, bracketed=bracketed.astype(bool), n_trials=n_trials, statistic=stat,
                          null_errors=err0, exposures=H, reconstruction_errors=err, tested=tested.astype(bool), max_kl_increase=delta,
                          test=tuple(int(v) for v in T), candidates=C, trace_values=trace_c, trace_profile=trace_g, timings=timings)
