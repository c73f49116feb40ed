"""Exposures to FIXED signatures, with bootstrap intervals (``csrc/salnmf_refit.h``).

With the signatures fixed the samples decouple: :func:`refit_exposures` solves every sample on its own -- start
``h_k = sum(x) / K``, the multiplicative ``update_H`` step, the sample's own KL divergence as the objective and the
sample's own convergence test -- so the exposures of a sample are a property of the sample and the signatures, not of the
cohort it arrives in.  With ``n_resamples = R > 0`` the same is done for R bootstrap resamples of the counts
(``resample_counts(counts, R, resample_seed)``, drawn on the device and never downloaded), and a second kernel reduces the
R exposures of every (sample, signature) to their mean and to order statistics.  There is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import time
from ctypes import c_double
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .anndata_compat import ANNDATA_TYPES
from .initialization import check_given_asignatures
from .resample import check_counts, check_seed

MAX_SIGNATURES = 96
MAX_FEATURES = 96
MAX_RESAMPLES = 1024  # the reduction sorts the R values of a (sample, signature) in one pass
MAX_QUANTILES = 16
DEFAULT_CHUNK_BYTES = 256 << 20
_ANNDATA = tuple(ANNDATA_TYPES)


@dataclass
class RefitResult:
    exposures: np.ndarray  # (N, K)
    reconstruction_errors: np.ndarray  # (N,): the sample's KL divergence where it stopped
    n_iterations: np.ndarray  # (N,) int32
    converged: np.ndarray  # (N,) bool
    exposures_quantiles: np.ndarray | None = None  # (Q, N, K): order statistics over the resamples
    exposures_mean: np.ndarray | None = None  # (N, K)
    n_iterations_resampled: np.ndarray | None = None  # (R, N)
    reconstruction_errors_resampled: np.ndarray | None = None  # (R, N)
    exposures_resampled: np.ndarray | None = None  # (R, N, K) with keep_resamples
    quantiles: tuple = ()
    timings: dict = field(default_factory=dict)


def quantile_indices(quantiles, n_resamples: int) -> np.ndarray:
    """Index into the R sorted values of each quantile, taken outward: ``floor(q (R - 1))`` for q <= 0.5, ``ceil`` above."""
    q = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    pos = q * float(n_resamples - 1)
    return np.clip(np.where(q <= 0.5, np.floor(pos), np.ceil(pos)), 0, n_resamples - 1).astype(np.int64)


def _check_int(name, value, minimum):
    if not isinstance(value, (int, np.integer)) or isinstance(value, bool) or int(value) < minimum:
        raise ValueError(f"'{name}' must be an integer >= {minimum}.")
    return int(value)


def normalize_signatures(signatures) -> np.ndarray:
    """``(K, V)`` float64 rows divided by their sums, or ``ValueError``: the rows must be finite, non-negative, of positive sum."""
    S = np.ascontiguousarray(signatures, dtype=np.float64)
    if S.ndim != 2:
        raise ValueError("'signatures' must be a matrix (signatures x features).")
    K, V = S.shape
    if not 1 <= K <= MAX_SIGNATURES:
        raise ValueError(f"refit_exposures handles 1 to {MAX_SIGNATURES} signatures, got {K}.")
    if not 1 <= V <= MAX_FEATURES:
        raise ValueError(f"refit_exposures handles 1 to {MAX_FEATURES} features, got {V}.")
    if not np.isfinite(S).all() or (S < 0).any():
        raise ValueError("Signatures must be finite and non-negative.")
    sums = S.sum(axis=1, keepdims=True)
    if not np.isfinite(sums).all() or (sums <= 0).any():
        raise ValueError("Every signature needs a positive sum.")
    return np.ascontiguousarray(S / sums)


def check_arguments(counts, signatures, n_resamples, resample_seed, quantiles, min_iterations, max_iterations, conv_test_freq, tol, chunk_bytes):
    """Everything :func:`refit_exposures` (and ``assign_signatures``) refuses before it touches a device, as ``ValueError``:
    returns ``(X, S, R, seed, min_it, max_it, freq, tol, q, chunk)`` ready for the C call."""
    if isinstance(counts, _ANNDATA) and isinstance(signatures, _ANNDATA):
        check_given_asignatures(signatures, counts, signatures.n_obs)
    X = np.ascontiguousarray(np.asarray(counts.X if isinstance(counts, _ANNDATA) else counts), dtype=np.float64)
    S = normalize_signatures(np.asarray(signatures.X if isinstance(signatures, _ANNDATA) else signatures))
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError("'counts' must be a matrix (samples x features) with at least one row.")
    N, V = X.shape
    K = S.shape[0]
    if S.shape[1] != V:
        raise ValueError(f"The signatures have {S.shape[1]} features, the counts {V}.")
    if not np.isfinite(X).all() or (X < 0).any():
        raise ValueError("Counts must be finite and non-negative.")
    R = _check_int("n_resamples", n_resamples, 0)
    if R > MAX_RESAMPLES:
        raise ValueError(f"'n_resamples' must be at most {MAX_RESAMPLES}: the reduction sorts a signature's resamples in one pass.")
    seed = check_seed(resample_seed)
    min_it, max_it = _check_int("min_iterations", min_iterations, 0), _check_int("max_iterations", max_iterations, 0)
    if max_it < min_it or max_it >= 2**31:
        raise ValueError("Need min_iterations <= max_iterations < 2**31.")
    freq = _check_int("conv_test_freq", conv_test_freq, 1)
    tol = float(tol)
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("'tol' must be finite and not negative.")
    q = np.ascontiguousarray(np.asarray(quantiles, dtype=np.float64).reshape(-1))
    if q.size > MAX_QUANTILES or not ((q >= 0) & (q <= 1)).all():
        raise ValueError(f"'quantiles' must hold at most {MAX_QUANTILES} values in [0, 1].")
    chunk = DEFAULT_CHUNK_BYTES if chunk_bytes is None else _check_int("chunk_bytes", chunk_bytes, 1)
    if R > 0:
        check_counts(X)
    return X, S, R, seed, min_it, max_it, freq, tol, q, chunk


def call_refit(symbol, model_args, X, S, R, seed, q, min_it, max_it, freq, tol, chunk, keep_resamples, device, t_start=None) -> dict:
    """One ``salnmf_*_refit_exposures`` call on checked arguments: the outputs' allocation, the call of ``symbol`` with
    ``model_args`` (the model's own arrays) after K, and the timings (``total_s`` from ``t_start``, the caller's start).  Returns the
    fields of a :class:`RefitResult`."""
    t_start = time.perf_counter() if t_start is None else t_start
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
    _lib.check(getattr(lib, symbol)(
        int(device), p(X), N, V, p(S), K, *(p(m) for m in model_args), R, seed, Q if R else 0, p(q), min_it, max_it, freq, tol, chunk,
        p(H), p(err), p(nit), p(conv), p(Hq), p(Hm), p(nit_r), p(err_r), p(Hr), ctypes.cast(ms, _lib._D),
    ))
    timings = {"resample_s": ms[0] / 1e3, "refit_s": ms[1] / 1e3, "reduce_s": ms[2] / 1e3, "refit_kernel_ms": ms[1],
               "n_chunks": int(ms[3]), "total_s": time.perf_counter() - t_start}
    return dict(exposures=H, reconstruction_errors=err, n_iterations=nit, converged=conv.astype(bool), exposures_quantiles=Hq,
                exposures_mean=Hm, n_iterations_resampled=nit_r, reconstruction_errors_resampled=err_r, exposures_resampled=Hr,
                quantiles=tuple(float(v) for v in q), timings=timings)


def refit_exposures(counts, signatures, n_resamples: int = 0, resample_seed: int = 0, quantiles=(0.025, 0.5, 0.975),
                    min_iterations: int = 500, max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7,
                    keep_resamples: bool = False, device: int = 0, chunk_bytes: int | None = None) -> RefitResult:
    """Exposures of every row of ``counts (N, V)`` to the fixed ``signatures (K, V)``, K <= 96 and V <= 96.

    The signature rows are divided by their sums and used as they are (never clipped).  Every sample is iterated and
    stopped on its own (module docstring); ``n_resamples`` adds the bootstrap: ``exposures_mean``, ``exposures_quantiles``
    (existing values: index ``floor(q (R - 1))`` of the sorted resamples for q <= 0.5, ``ceil`` above) and, with
    ``keep_resamples``, every resample's exposures.  ``chunk_bytes`` bounds the device buffer the resamples are drawn into
    (default 256 MiB; the result does not depend on it).  Anything out of range is a ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, S, R, seed, min_it, max_it, freq, tol, q, chunk = check_arguments(counts, signatures, n_resamples, resample_seed, quantiles, min_iterations,
                                                                         max_iterations, conv_test_freq, tol, chunk_bytes)
    return RefitResult(**call_refit("salnmf_refit_exposures", (), X, S, R, seed, q, min_it, max_it, freq, tol, chunk, keep_resamples, device, t_start))
