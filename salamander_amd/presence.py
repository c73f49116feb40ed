"""Is signature s present in this sample?  A calibrated p-value per (sample, tested signature) (``csrc/salnmf_presence.h``).

:func:`assign_signatures` decides on a signature by comparing the rise of the sample's KL divergence with a fixed
``max_kl_increase`` -- "a parameter, not a measurement": under the null the exposure sits on the boundary ``h_s >= 0``, and at a
few hundred mutations no asymptotic table holds.  :func:`signature_presence_test` measures instead.  For every sample and every
tested signature s it fits the sample with and without s (two dense solves on the candidate set C and on C without s), takes
``statistic = f0 - f1``, draws ``n_draws`` count vectors of the sample's own total from the fit *without* s, puts every draw
through the same two solves, and reports where the observed statistic falls among the null ones:
``p_value = (1 + n_exceed) / (n_draws + 1)``.  Everything runs on the device; there is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import time
from ctypes import c_double
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .assign import check_sets
from .gof import check_integer_counts, check_n_draws
from .refit import check_arguments


@dataclass
class PresenceResult:
    statistic: np.ndarray  # (N, S): f0 - f1, half the likelihood-ratio statistic; NaN where the pair is untested
    p_value: np.ndarray  # (N, S): (1 + n_exceed) / (B + 1); NaN where the pair is untested
    n_exceed: np.ndarray  # (N, S) int32: draws b with null_statistics[b, n, j] >= statistic[n, j]
    tested: np.ndarray  # (N, S) bool: s is a candidate of the sample and not its only one
    exposures: np.ndarray  # (N, K): the alternative fit, on the candidate set (NaN rows where no pair of the sample is tested)
    reconstruction_errors: np.ndarray  # (N,): f1
    null_exposures: np.ndarray  # (N, S, K): the fit without s, exactly 0.0 at s
    null_errors: np.ndarray  # (N, S): f0
    null_statistics: np.ndarray  # (B, N, S)
    null_mean: np.ndarray  # (N, S): the sum of null_statistics[:, n, j] in ascending b, divided by B
    n_iterations: np.ndarray  # (N, S, 2) int32: the observed solves, alternative and null
    converged: np.ndarray  # (N, S, 2) bool
    null_n_iterations: np.ndarray  # (B, N, S, 2) int32
    test: tuple = ()
    candidates: np.ndarray | None = None  # (N, K) bool as applied, None = every signature
    draws: np.ndarray | None = None  # (B, N, S, V) with keep_draws
    timings: dict = field(default_factory=dict)


def check_test(test, K: int) -> np.ndarray:
    """``test`` as an int32 array of distinct signature indices in [0, K), or ``ValueError``."""
    message = f"'test' must be a non-empty list of distinct signature indices in [0, {K})."
    if isinstance(test, (str, bytes)) or not hasattr(test, "__len__") or len(test) == 0:
        raise ValueError(message)
    values = list(test)
    if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in values):
        raise ValueError(message)
    if any(not 0 <= int(v) < K for v in values) or len({int(v) for v in values}) != len(values):
        raise ValueError(message)
    return np.array([int(v) for v in values], dtype=np.int32)


def check_presence_arguments(counts, signatures, test, n_draws, seed, candidates, min_iterations, max_iterations, conv_test_freq, tol, chunk_bytes):
    """What :func:`signature_presence_test` checks before it touches a device ->
    ``(X, W, T, C, B, seed, min_it, max_it, freq, tol, chunk)``."""
    X, W, _, seed, min_it, max_it, freq, tol, _, chunk = check_arguments(counts, signatures, 0, seed, (), min_iterations, max_iterations,
                                                                        conv_test_freq, tol, chunk_bytes)
    if max_it % freq != 0:
        raise ValueError("'max_iterations' must be a multiple of 'conv_test_freq': the two solves of a pair follow one another on the device.")
    check_integer_counts(X)
    B = check_n_draws(n_draws)
    T = check_test(test, W.shape[0])
    C, _, _ = check_sets(candidates, None, False, X.shape[0], W.shape[0])
    return X, W, T, C, B, seed, min_it, max_it, freq, tol, chunk


class PresenceOutputs:
    """The arrays ``salnmf_signature_presence`` fills, in the C order, and the :class:`PresenceResult` made of them."""

    def __init__(self, N, V, K, S, B, keep_draws):
        f64 = lambda *shape: np.empty(shape, dtype=np.float64)  # noqa: E731
        i32 = lambda *shape: np.empty(shape, dtype=np.int32)  # noqa: E731
        self.B = B
        self.tested = np.zeros((N, S), dtype=np.uint8)
        self.stat, self.mean, self.H, self.err, self.H0, self.err0 = f64(N, S), f64(N, S), f64(N, K), f64(N), f64(N, S, K), f64(N, S)
        self.exceed, self.nit, self.conv = i32(N, S), i32(N, S, 2), i32(N, S, 2)
        self.stat_b, self.nit_b = f64(B, N, S), i32(B, N, S, 2)
        self.drawn = f64(B, N, S, V) if keep_draws else None

    def pointers(self):
        p = _lib.pointer
        return (p(self.tested), p(self.stat), p(self.exceed), p(self.mean), p(self.H), p(self.err), p(self.H0), p(self.err0), p(self.nit),
                p(self.conv), p(self.stat_b), p(self.nit_b), p(self.drawn))

    def result(self, T, C, ms, total_s) -> PresenceResult:
        tested = self.tested.astype(bool)
        timings = {"draw_s": ms[0] / 1e3, "solve_s": ms[1] / 1e3, "reduce_s": ms[2] / 1e3, "presence_kernel_ms": ms[1], "n_chunks": int(ms[3]),
                   "total_s": total_s}
        p_value = np.where(tested, (1 + self.exceed.astype(np.int64)) / (self.B + 1), np.nan)
        return PresenceResult(statistic=self.stat, p_value=p_value, n_exceed=self.exceed, tested=tested, exposures=self.H, reconstruction_errors=self.err,
                              null_exposures=self.H0, null_errors=self.err0, null_statistics=self.stat_b, null_mean=self.mean, n_iterations=self.nit,
                              converged=self.conv.astype(bool), null_n_iterations=self.nit_b, test=tuple(int(v) for v in T), candidates=C,
                              draws=self.drawn, timings=timings)


def call_presence(symbol, model_args, X, W, T, C, B, seed, min_it, max_it, freq, tol, chunk, keep_draws, device, count_failed=False):
    """One ``salnmf_*signature_presence`` call on checked arguments: the outputs' allocation and the call of ``symbol`` with
    ``model_args`` (the model's own arrays) after K and, with ``count_failed``, a trailing output for the rows no draw could be
    made for.  Returns ``(the PresenceOutputs, the four timings, that count)``."""
    (N, V), K, S = X.shape, W.shape[0], int(T.size)
    lib = _lib.load_with_device()
    out = PresenceOutputs(N, V, K, S, B, keep_draws)
    Cb = None if C is None else C.astype(np.uint8)
    failed = np.zeros(1, dtype=np.int32)
    ms = (c_double * 4)()
    p = _lib.pointer
    _lib.check(getattr(lib, symbol)(
        int(device), p(X), N, V, p(W), K, *(p(m) for m in model_args), p(T), S, p(Cb), B, seed, min_it, max_it, freq, tol, chunk, *out.pointers(),
        ctypes.cast(ms, _lib._D), *([p(failed)] if count_failed else []),
    ))
    return out, ms, int(failed[0])


def signature_presence_test(counts, signatures, test, n_draws: int = 200, seed: int = 0, candidates=None, min_iterations: int = 500,
                            max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7, chunk_bytes: int | None = None,
                            keep_draws: bool = False, device: int = 0) -> PresenceResult:
    """The bootstrap likelihood-ratio test of every signature in ``test`` in every row of ``counts (N, V)`` against the fixed
    ``signatures (K, V)``, K <= 96 and V <= 96.

    With C the sample's candidate set (``candidates``: ``None``, or a boolean mask of shape (K,) or (N, K), as
    :func:`assign_signatures` takes it) and s = ``test[j]``: the alternative is
    ``assign_signatures(x, signatures, candidates=C, required=C, ...)`` and the null the same call on C without s, bit for bit
    with the same iteration arguments; ``statistic[n, j] = f0 - f1``.  Null draw b comes from the fit without s, with the
    sample's own total, and goes through the same two solves.  A pair with s outside C or C = {s} is untested: NaN, ``tested``
    False, no draw and no solve.  ``p_value`` is per sample and per signature, conditional on the sample's total, uncorrected
    for multiplicity and never below ``1 / (n_draws + 1)``.  ``max_iterations`` must be a multiple of ``conv_test_freq``;
    ``chunk_bytes`` bounds the device buffer the draws are written into (default 256 MiB; the result does not depend on it).
    The counts are non-negative integers with row totals below 2**32; anything out of range is a ``ValueError`` before the
    device is touched."""
    t_start = time.perf_counter()
    X, W, T, C, B, seed, min_it, max_it, freq, tol, chunk = check_presence_arguments(counts, signatures, test, n_draws, seed, candidates, min_iterations,
                                                                                     max_iterations, conv_test_freq, tol, chunk_bytes)
    out, ms, _ = call_presence("salnmf_signature_presence", (), X, W, T, C, B, seed, min_it, max_it, freq, tol, chunk, keep_draws, device)
    return out.result(T, C, ms, time.perf_counter() - t_start)
