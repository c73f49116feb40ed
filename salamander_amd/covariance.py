"""Which exposures trade against each other in a sample?  The information matrix of a sample's exposures at the fit, its inverse,
and what the inverse says about confounding (``csrc/salnmf_information.h``).

:func:`exposure_intervals` shows that an exposure is poorly determined, but not by what.  :func:`exposure_covariance` gives the
joint second-order picture at the fit: per sample the information matrix ``J = W diag(d) W^T`` of the active signatures, and from
its inverse the Wald standard error of every exposure, the factor by which the other signatures inflate its variance, and the
signature it is most strongly confounded with.  These are local statements at the supplied exposures -- no joint region, no
correction for the boundary at 0.  Everything runs on the device; there is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import time
from ctypes import c_double
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .refit import check_arguments, refit_exposures

INFORMATION = {"observed": 0, "expected": 1}


@dataclass
class CovarianceResult:
    standard_errors: np.ndarray  # (N, K): sqrt((C^-1)_kk / J_kk); NaN where k is inactive or the sample is singular
    inflation: np.ndarray  # (N, K): (C^-1)_kk, exactly 1 for a lone signature and for one orthogonal to the rest
    information_diag: np.ndarray  # (N, K): J_kk
    max_abs_correlation: np.ndarray  # (N, K): the largest |corr_kl| over the active l != k; NaN where there is none
    most_confounded: np.ndarray  # (N, K) int32: its index, the smallest on a tie; -1 where undefined
    min_pivot_value: np.ndarray  # (N,): the smallest squared pivot of the Cholesky factor of C; NaN without an active signature
    singular: np.ndarray  # (N,) bool: a squared pivot was <= min_pivot
    n_active: np.ndarray  # (N,) int32
    exposures: np.ndarray  # (N, K) as used
    active: np.ndarray  # (N, K) bool as used
    information: str = "observed"
    min_pivot: float = 1e-10
    correlation: np.ndarray | None = None  # (N, K, K) with return_correlation: unit diagonal on the active set, NaN elsewhere
    timings: dict = field(default_factory=dict)


def check_exposures(exposures, N: int, K: int) -> np.ndarray:
    """``exposures`` as a contiguous float64 ``(N, K)`` array of finite numbers >= 0, or ``ValueError``."""
    message = f"'exposures' must hold finite numbers >= 0 in shape ({N}, {K})."
    if isinstance(exposures, (str, bytes)):
        raise ValueError(message)
    try:
        raw = np.asarray(exposures)
    except (TypeError, ValueError):
        raise ValueError(message) from None
    if raw.dtype == bool or not (np.issubdtype(raw.dtype, np.integer) or np.issubdtype(raw.dtype, np.floating)):
        raise ValueError(message)
    H = np.ascontiguousarray(raw, dtype=np.float64)
    if H.shape != (N, K) or not np.isfinite(H).all() or (H < 0.0).any():
        raise ValueError(message)
    return H


def check_active(active, H: np.ndarray) -> np.ndarray:
    """``active`` as a contiguous bool ``(N, K)`` array; ``None`` is ``exposures > 0``."""
    N, K = H.shape
    if active is None:
        return np.ascontiguousarray(H > 0.0)
    m = np.asarray(active)
    if m.dtype != np.bool_:
        raise ValueError(f"'active' must be a boolean array, got dtype {m.dtype}.")
    if m.shape == (K,):
        m = np.broadcast_to(m, (N, K))
    elif m.shape != (N, K):
        raise ValueError(f"'active' must have shape ({K},) or ({N}, {K}), got {m.shape}.")
    return np.ascontiguousarray(m)


def exposure_covariance(counts, signatures, exposures=None, active=None, information: str = "observed", min_pivot: float = 1e-10,
                        return_correlation: bool = False, device: int = 0, chunk_bytes: int | None = None) -> CovarianceResult:
    """Wald standard errors and signature confounding of every row of ``counts (N, V)`` at ``exposures (N, K)`` to the fixed
    ``signatures (K, V)``, K <= 96 and V <= 96.

    Counts and signatures are checked and normalised as :func:`refit_exposures` does; ``exposures=None`` calls
    ``refit_exposures(counts, signatures)`` at its defaults and uses the result.  ``active`` is a bool mask of shape (N, K) or
    (K,), by default ``exposures > 0``: every signature after a dense refit, the support after :func:`assign_signatures`.  With
    ``x = max(row, EPSILON)`` and the model mean ``p_v = max(sum_k W[k, v] h_k, EPSILON)`` over all k as supplied, the
    information matrix of the sample is ``J[k, l] = sum_v W[k, v] W[l, v] d_v`` on the active k, with ``d_v = x_v / p_v**2`` for
    ``information="observed"`` (the Hessian of the sample's KL divergence, that is of its Poisson negative log-likelihood) and
    ``d_v = 1 / p_v`` for ``"expected"``.  It is scaled to a unit diagonal, ``C = D^-1/2 J D^-1/2`` with ``D = diag(J)``, and
    factored ``C = L L^T`` in the natural order of k without pivoting; ``min_pivot_value`` is the smallest ``L[k, k]**2``, and a
    sample is ``singular`` as soon as a squared pivot is ``<= min_pivot`` -- a number in (0, 1); the default 1e-10 reads "a
    variance inflation above 1e10 is unidentifiable".

    ``standard_errors = sqrt((C^-1)_kk / J_kk)``; ``inflation = (C^-1)_kk`` is the factor by which the other active signatures
    inflate the variance of k; ``information_diag = J_kk``; ``max_abs_correlation`` and ``most_confounded`` give for each k the
    largest ``|corr_kl|`` over the active ``l != k`` and its index (the smallest on a tie, -1 where undefined), with
    ``corr_kl = (C^-1)_kl / sqrt((C^-1)_kk (C^-1)_ll)``; ``return_correlation=True`` adds the whole ``correlation (N, K, K)``.
    Every per-signature entry is NaN where k is inactive, where the sample is singular and where it has no active signature; a
    lone active signature has no correlation (NaN, -1).  A sample's results depend on that sample alone: not on N, its
    neighbours, ``chunk_bytes`` (the device buffer of the correlations, default 256 MiB) or ``return_correlation``.  Anything out
    of range is a ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, W, _, _, _, _, _, _, _, chunk = check_arguments(counts, signatures, 0, 0, (), 0, 0, 1, 0.0, chunk_bytes)
    (N, V), K = X.shape, W.shape[0]
    if not isinstance(information, str) or information not in INFORMATION:
        raise ValueError("'information' must be \"observed\" or \"expected\".")
    if isinstance(min_pivot, (bool, np.bool_, str)) or not isinstance(min_pivot, (int, float, np.integer, np.floating)) \
            or not np.isfinite(min_pivot) or not 0.0 < min_pivot < 1.0:
        raise ValueError("'min_pivot' must be a finite number in (0, 1).")
    if not isinstance(return_correlation, (bool, np.bool_)):
        raise ValueError("'return_correlation' must be True or False.")
    refit_s = 0.0
    if exposures is None:
        fit = refit_exposures(counts, signatures, device=device)  # (the arguments as given: the same bits as the caller's own refit)
        exposures, refit_s = fit.exposures, fit.timings["total_s"]
    H = check_exposures(exposures, N, K)
    A = check_active(active, H)
    lib = _lib.load_with_device()
    # (the library fills every entry)
    se, infl, info, maxc = (np.full((N, K), np.nan) for _ in range(4))
    conf = np.full((N, K), -1, dtype=np.int32)
    minp = np.full(N, np.nan)
    sing, nact = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    corr = np.full((N, K, K), np.nan) if return_correlation else None
    ms = (c_double * 2)()
    p = _lib.pointer
    _lib.check(lib.salnmf_exposure_covariance(
        int(device), p(X), N, V, p(W), K, p(H), p(A.view(np.uint8)), INFORMATION[information], float(min_pivot), chunk, p(se), p(infl), p(info), p(maxc),
        p(conf), p(minp), p(sing), p(nact), p(corr), ctypes.cast(ms, _lib._D),
    ))
    timings = {"information_kernel_ms": ms[0], "n_chunks": int(ms[1]), "refit_s": refit_s, "total_s": time.perf_counter() - t_start}
    return CovarianceResult(standard_errors=se, inflation=infl, information_diag=info, max_abs_correlation=maxc, most_confounded=conf,
                            min_pivot_value=minp, singular=sing.astype(bool), n_active=nact, exposures=H, active=A, information=information,
                            min_pivot=float(min_pivot), correlation=corr, timings=timings)
