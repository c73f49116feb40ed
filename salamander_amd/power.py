"""Could the presence test have seen signature s in this sample?  Detection power and limit per (sample, tested signature)
(``csrc/salnmf_power.h``).

"SBS3: p = 0.31" from :func:`signature_presence_test` cannot be read without knowing whether the test could have found SBS3
in this sample at all: 300 mutations on a flat background do not show a 10 % share at any p-value, 30 000 show 2 %.
:func:`signature_power` runs the presence test and then, for every tested pair and every share in ``shares``, plants the
signature at that share of the pair's null fit, draws ``n_alt_draws`` count vectors of the sample's own total from the planted
model, puts every draw through the presence test's two solves and counts how many of them the test would have called at level
``alpha`` against the pair's own null distribution.  Everything runs on the device; there is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import time
from ctypes import c_double
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .presence import PresenceOutputs, PresenceResult, check_presence_arguments

MAX_SHARES = 64  # salnmf_power.h: POWER_MAX_SHARES
MAX_ALT_DRAWS = 65536  # salnmf_power.h: POWER_MAX_DRAWS


@dataclass
class PowerResult:
    presence: PresenceResult  # bit for bit signature_presence_test's for the same arguments and seed
    shares: np.ndarray  # (L,)
    power: np.ndarray  # (L, N, S): n_detected / A; NaN where the pair is untested
    detection_limit: np.ndarray  # (N, S): the smallest share with power >= target_power; NaN if none (or untested)
    n_detected: np.ndarray  # (L, N, S) int32: draws a with alt_statistics not NaN and alt_n_exceed <= max_exceed
    alt_mean: np.ndarray  # (L, N, S): the sum of alt_statistics[l, :, n, j] in ascending a, divided by A
    planted_exposures: np.ndarray  # (L, N, S, K): (1 - share) * null_exposures off s, share * sum(null_exposures) at s
    alt_statistics: np.ndarray  # (L, A, N, S)
    alt_n_iterations: np.ndarray  # (L, A, N, S, 2) int32
    alt_n_exceed: np.ndarray  # (L, A, N, S) int32: null draws b with null_statistics[b, n, j] >= alt_statistics[l, a, n, j]
    max_exceed: int = 0  # the largest m with (1 + m) / (B + 1) <= alpha
    alpha: float = 0.05
    target_power: float = 0.8
    alt_draws: np.ndarray | None = None  # (L, A, N, S, V) with keep_draws
    timings: dict = field(default_factory=dict)


def check_shares(shares) -> np.ndarray:
    """``shares`` as a float64 array of 1 to 64 strictly ascending values in [0, 1), or ``ValueError``."""
    message = f"'shares' must be 1 to {MAX_SHARES} strictly ascending numbers in [0, 1)."
    if isinstance(shares, (str, bytes)) or not hasattr(shares, "__len__") or not 1 <= len(shares) <= MAX_SHARES:
        raise ValueError(message)
    values = list(shares)
    if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) for v in values):
        raise ValueError(message)
    out = np.array([float(v) for v in values], dtype=np.float64)
    if not np.isfinite(out).all() or (out < 0.0).any() or (out >= 1.0).any() or (np.diff(out) <= 0.0).any():
        raise ValueError(message)
    return out


def _integer(value, lo: int, hi: int, name: str) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"'{name}' must be an integer in [{lo}, {hi}].")
    return int(value)


def _probability(value, name: str) -> float:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) or not 0.0 < float(value) <= 1.0:
        raise ValueError(f"'{name}' must be a number in (0, 1].")
    return float(value)


def max_exceed_for(alpha: float, n_draws: int) -> int:
    """The largest integer m >= 0 with ``(1 + m) / (n_draws + 1) <= alpha``, the presence test's own p-value expression
    evaluated in Python floats: ``n_exceed <= m`` is exactly ``p_value <= alpha``.  ``ValueError`` if there is none."""
    B = int(n_draws)
    m = min(B, int(alpha * (B + 1)))  # within one of the answer; the expression itself decides
    while m < B and (1 + (m + 1)) / (B + 1) <= alpha:
        m += 1
    while m >= 0 and not (1 + m) / (B + 1) <= alpha:
        m -= 1
    if m < 0:
        raise ValueError(f"'alpha' = {alpha} cannot be reached with {B} null draws: the smallest p-value is 1 / {B + 1}.")
    return m


def detection_limit_of(shares: np.ndarray, power: np.ndarray, target_power: float) -> np.ndarray:
    """(N, S): the smallest of the ascending ``shares`` whose ``power[l]`` is at least ``target_power``; NaN if none."""
    with np.errstate(invalid="ignore"):
        passed = power >= target_power  # NaN: False
    first = passed.argmax(axis=0)
    return np.where(passed.any(axis=0), shares[first], np.nan)


def signature_power(counts, signatures, test, shares=(0.0, 0.02, 0.05, 0.1, 0.2), n_draws: int = 200, n_alt_draws: int = 200, alpha: float = 0.05,
                    target_power: float = 0.8, candidates=None, seed: int = 0, keep_draws: bool = False, min_iterations: int = 500,
                    max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7, chunk_bytes: int | None = None,
                    device: int = 0) -> PowerResult:
    """Detection power of :func:`signature_presence_test` for every signature in ``test``, in every row of ``counts (N, V)``, at
    every share in ``shares`` (strictly ascending, in [0, 1)), and the smallest share detected with ``target_power``.

    The presence test runs first, unchanged: ``.presence`` is bit for bit what :func:`signature_presence_test` returns for the
    same arguments and seed, and pairs it leaves untested stay untested here (NaN, 0 in the integers, no cost).  For a tested
    pair (n, s) with null fit h0 (``presence.null_exposures``) and share pi, the planted exposures are ``(1 - pi) * h0`` off s
    and ``pi * sum(h0)`` at s; alternative draw a is one model draw of the sample's own total from them, with random numbers
    that depend on (seed, n, s, a) only -- all shares of a pair use the same ones, so the power curve is smooth in the share and
    a share's result does not depend on which other shares are asked for.  Every draw goes through the presence test's two
    solves; it is *detected* when at most ``max_exceed`` of the pair's ``n_draws`` null statistics reach its statistic, with
    ``max_exceed`` the largest m with ``(1 + m) / (n_draws + 1) <= alpha`` -- exactly "the presence test would have given
    p <= alpha against this null".  ``power = n_detected / n_alt_draws``; ``detection_limit`` is the smallest share with
    ``power >= target_power``, NaN if there is none.  ``alpha * (n_draws + 1) < 1`` is refused: no p-value can be that small.

    Limits.  The critical value comes from the null drawn from the *observed* sample's h0; it is not re-estimated for every
    alternative draw, which would take a nested bootstrap of ``n_alt_draws * n_draws`` draws per share.  Power at share 0 is
    therefore a direct check of that approximation and should sit near ``alpha``.  The planted signature displaces the fitted
    background proportionally.  Everything is conditional on the sample's total."""
    t_start = time.perf_counter()
    X, W, T, C, B, seed, min_it, max_it, freq, tol, chunk = check_presence_arguments(counts, signatures, test, n_draws, seed, candidates, min_iterations,
                                                                                     max_iterations, conv_test_freq, tol, chunk_bytes)
    pi = check_shares(shares)
    A = _integer(n_alt_draws, 1, MAX_ALT_DRAWS, "n_alt_draws")
    alpha, target = _probability(alpha, "alpha"), _probability(target_power, "target_power")
    m = max_exceed_for(alpha, B)
    (N, V), K, S, L = X.shape, W.shape[0], int(T.size), int(pi.size)
    lib = _lib.load_with_device()

    out = PresenceOutputs(N, V, K, S, B, keep_draws)
    Hp, stat_a, mean_a = np.empty((L, N, S, K)), np.empty((L, A, N, S)), np.empty((L, N, S))
    nit_a, exceed_a, n_det = np.empty((L, A, N, S, 2), dtype=np.int32), np.empty((L, A, N, S), dtype=np.int32), np.empty((L, N, S), dtype=np.int32)
    drawn_a = np.empty((L, A, N, S, V)) if keep_draws else None
    Cb = None if C is None else C.astype(np.uint8)
    ms = (c_double * 9)()
    p = _lib.pointer
    _lib.check(lib.salnmf_signature_power(
        int(device), p(X), N, V, p(W), K, p(T), S, p(Cb), B, seed, min_it, max_it, freq, tol, chunk, p(pi), L, A, m, *out.pointers(),
        p(Hp), p(stat_a), p(nit_a), p(exceed_a), p(n_det), p(mean_a), p(drawn_a), ctypes.cast(ms, _lib._D),
    ))
    total_s = time.perf_counter() - t_start
    presence = out.result(T, C, ms, total_s)
    power = np.where(presence.tested[None], n_det / A, np.nan)
    timings = {"plant_s": ms[4] / 1e3, "alt_draw_s": ms[5] / 1e3, "alt_solve_s": ms[6] / 1e3, "power_reduce_s": ms[7] / 1e3,
               "alt_presence_kernel_ms": ms[6], "n_alt_chunks": int(ms[8]), "total_s": total_s}
    return PowerResult(presence=presence, shares=pi, power=power, detection_limit=detection_limit_of(pi, power, target), n_detected=n_det,
                       alt_mean=mean_a, planted_exposures=Hp, alt_statistics=stat_a, alt_n_iterations=nit_a, alt_n_exceed=exceed_a, max_exceed=m,
                       alpha=alpha, target_power=target, alt_draws=drawn_a, timings=timings)
