"""Does the catalogue explain the sample at all?  A parametric-bootstrap p-value per sample (``csrc/salnmf_gof.h``).

:func:`refit_exposures` says how much of each signature a sample carries; its ``reconstruction_errors`` -- the sample's KL
divergence -- cannot be read on its own, because its distribution under a correct catalogue depends on the sample's mutation
count and on the number of signatures.  :func:`goodness_of_fit` calibrates it: for every sample it draws ``n_draws`` count
vectors of the sample's own total from the sample's own fitted model (on the device, from the exposures where the refit left
them), refits each one exactly as the sample was refitted, and reports where the observed divergence falls among the null
ones: ``p_value = (1 + n_exceed) / (n_draws + 1)``.  :func:`draw_model_counts` is the draw alone.  There is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import time
from ctypes import c_double
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .refit import check_arguments, normalize_signatures
from .resample import _int_in_range, check_seed

MAX_DRAWS = 65536


@dataclass
class GofResult:
    exposures: np.ndarray  # (N, K): the observed dense refit, as refit_exposures returns it
    reconstruction_errors: np.ndarray  # (N,)
    n_iterations: np.ndarray  # (N,) int32
    converged: np.ndarray  # (N,) bool
    n_exceed: np.ndarray  # (N,) int32: draws b with null_errors[b, n] >= reconstruction_errors[n]
    p_value: np.ndarray  # (N,): (1 + n_exceed) / (B + 1)
    null_mean: np.ndarray  # (N,): the sum of null_errors[:, n] in ascending b, divided by B
    null_errors: np.ndarray  # (B, N)
    null_n_iterations: np.ndarray  # (B, N) int32
    draws: np.ndarray | None = None  # (B, N, V) with keep_draws
    timings: dict = field(default_factory=dict)


def check_n_draws(n_draws) -> int:
    return _int_in_range(n_draws, 1, MAX_DRAWS, f"'n_draws' must be an integer in [1, {MAX_DRAWS}].")


def check_integer_counts(X) -> np.ndarray:
    """``X`` unchanged, or ``ValueError`` naming the first row no model can be drawn for: an entry that is not an integer
    value (negative and non-finite entries are refused before), or a row total of 2**32 or more."""
    bad = X != np.floor(X)
    rows = np.flatnonzero(bad.any(axis=1))
    if rows.size:
        n = int(rows[0])
        v = int(np.flatnonzero(bad[n])[0])
        raise ValueError(f"goodness_of_fit needs integer counts: row {n}, column {v} holds {X[n, v]:g}.")
    rows = np.flatnonzero(X.sum(axis=1) >= 2.0**32)
    if rows.size:
        raise ValueError(f"goodness_of_fit needs row totals below 2**32: row {int(rows[0])} sums to {X[int(rows[0])].sum():.0f}.")
    return X


def check_model(exposures, signatures):
    """``(H (N, K), S (K, V))`` of a fitted model, or ``ValueError``: the signature rows divided by their sums, the exposures
    finite and non-negative with one column per signature and at least one row."""
    S = normalize_signatures(signatures)
    K = S.shape[0]
    H = np.ascontiguousarray(exposures, dtype=np.float64)
    if H.ndim != 2 or H.shape[0] < 1 or H.shape[1] != K:
        raise ValueError(f"'exposures' must be a matrix (samples x {K} signatures) with at least one row.")
    if not np.isfinite(H).all() or (H < 0).any():
        raise ValueError("Exposures must be finite and non-negative.")
    return H, S


def draw_model_counts(exposures, signatures, totals, n_draws: int, seed: int = 0, device: int = 0) -> np.ndarray:
    """``n_draws`` count matrices drawn from the model ``exposures (N, K) @ signatures (K, V)``: ``(n_draws, N, V)`` float64 of
    integer values, row n of every draw a multinomial draw of ``totals[n]`` trials from the spectrum of row n (the contract:
    ``include/salnmf.h``).  The signature rows are divided by their sums; the exposures are finite and non-negative, the totals
    integers in [0, 2**32).  The same bits on every run, and draw b does not depend on ``n_draws``."""
    H, S = check_model(exposures, signatures)
    (N, K), V = H.shape, S.shape[1]
    T = np.ascontiguousarray(totals, dtype=np.float64)
    if T.shape != (H.shape[0],):
        raise ValueError("'totals' must hold one trial count per row of the exposures.")
    if not np.isfinite(T).all() or (T < 0).any() or (T != np.floor(T)).any() or (T >= 2.0**32).any():
        raise ValueError("Totals must be non-negative integers below 2**32.")
    B, seed = check_n_draws(n_draws), check_seed(seed)
    lib = _lib.load_with_device()
    out = np.empty((B, N, V), dtype=np.float64)
    p = _lib.pointer
    _lib.check(lib.salnmf_draw_model_counts(int(device), p(H), N, K, p(S), V, p(T), B, seed, p(out)))
    return out


def call_gof(symbol, model_args, X, S, B, seed, min_it, max_it, freq, tol, chunk, keep_draws, device, t_start, count_failed=False):
    """One ``salnmf_*goodness_of_fit`` call on checked arguments: the outputs' allocation, the call of ``symbol`` with
    ``model_args`` (the model's own arrays) after K and, with ``count_failed``, a trailing output for the rows no draw could
    be made for.  Returns ``(the fields of a GofResult, that count)``."""
    (N, V), K = X.shape, S.shape[0]
    lib = _lib.load_with_device()

    H = np.empty((N, K), dtype=np.float64)
    err = np.empty(N, dtype=np.float64)
    nit = np.empty(N, dtype=np.int32)
    conv = np.empty(N, dtype=np.int32)
    exceed = np.empty(N, dtype=np.int32)
    mean = np.empty(N, dtype=np.float64)
    err_b = np.empty((B, N), dtype=np.float64)
    nit_b = np.empty((B, N), dtype=np.int32)
    drawn = np.empty((B, N, V), dtype=np.float64) if keep_draws else None
    failed = np.zeros(1, dtype=np.int32)
    ms = (c_double * 4)()
    p = _lib.pointer
    _lib.check(getattr(lib, symbol)(
        int(device), p(X), N, V, p(S), K, *(p(m) for m in model_args), B, seed, min_it, max_it, freq, tol, chunk,
        p(H), p(err), p(nit), p(conv), p(exceed), p(mean), p(err_b), p(nit_b), p(drawn), ctypes.cast(ms, _lib._D), *([p(failed)] if count_failed else []),
    ))
    timings = {"draw_s": ms[0] / 1e3, "refit_s": ms[1] / 1e3, "reduce_s": ms[2] / 1e3, "refit_kernel_ms": ms[1], "n_chunks": int(ms[3]),
               "total_s": time.perf_counter() - t_start}
    fields = dict(exposures=H, reconstruction_errors=err, n_iterations=nit, converged=conv.astype(bool), n_exceed=exceed,
                  p_value=(1 + exceed.astype(np.int64)) / (B + 1), null_mean=mean, null_errors=err_b, null_n_iterations=nit_b, draws=drawn,
                  timings=timings)
    return fields, int(failed[0])


def goodness_of_fit(counts, signatures, n_draws: int = 200, seed: int = 0, min_iterations: int = 500, max_iterations: int = 10000,
                    conv_test_freq: int = 10, tol: float = 1e-7, chunk_bytes: int | None = None, keep_draws: bool = False,
                    device: int = 0) -> GofResult:
    """The parametric-bootstrap test of every row of ``counts (N, V)`` against the fixed ``signatures (K, V)``, K <= 96 and V <= 96.

    The observed fit is ``refit_exposures(counts, signatures, ...)`` bit for bit.  Draw b is
    ``draw_model_counts(exposures, signatures, counts.sum(1), n_draws, seed)[b]`` and its refit
    ``refit_exposures(draws[b], signatures, ...)``, bit for bit, with the same iteration arguments: the data and the null go
    through one procedure.  ``p_value`` is ``(1 + n_exceed) / (n_draws + 1)``: small where the catalogue does not explain the
    sample, never below ``1 / (n_draws + 1)``, and conditional on the sample's own total.  Both sides are dense refits.
    ``chunk_bytes`` bounds the device buffer the draws are written into (default 256 MiB; the result does not depend on it).
    The counts are non-negative integers with row totals below 2**32; anything out of range is a ``ValueError`` before the
    device is touched."""
    t_start = time.perf_counter()
    X, S, _, seed, min_it, max_it, freq, tol, _, chunk = check_arguments(counts, signatures, 0, seed, (), min_iterations, max_iterations,
                                                                        conv_test_freq, tol, chunk_bytes)
    check_integer_counts(X)
    B = check_n_draws(n_draws)
    fields, _ = call_gof("salnmf_goodness_of_fit", (), X, S, B, seed, min_it, max_it, freq, tol, chunk, keep_draws, device, t_start)
    return GofResult(**fields)
