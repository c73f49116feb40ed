"""Which of the FIXED signatures are active in each sample (``csrc/salnmf_assign.h``).

:func:`refit_exposures` is dense by construction: every signature starts at ``sum(x) / K`` and the step clips at EPSILON, so
no exposure is ever zero.  :func:`assign_signatures` answers with a sparse support per sample by backward elimination, all
of it inside one kernel: the dense refit first (phase 0, bit for bit ``refit_exposures``), then rounds in which the active,
not yet protected signature of smallest exposure is set to 0.0 and the rest is solved again; the removal is kept if the
sample's KL divergence rose by at most ``max_kl_increase``, otherwise the signature is protected for good.  With
``n_resamples = R > 0`` the whole procedure also runs for R bootstrap resamples of the counts and the device reduces them to
a selection frequency per (sample, signature) and to the mean and order statistics of the exposures, zeros included.  There
is no CPU fallback.

``candidates`` restricts the catalogue per sample (the start value and every solve see the candidate signatures only),
``required`` names signatures that are never tried for removal, and ``readd=True`` follows the backward rounds with a
re-addition pass over the removed candidates, all inside the same kernel launch.
"""

from __future__ import annotations

import ctypes
import time
from ctypes import c_double
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .refit import check_arguments


@dataclass
class AssignResult:
    exposures: np.ndarray  # (N, K), exactly 0.0 off the support
    active: np.ndarray  # (N, K) bool
    reconstruction_errors: np.ndarray  # (N,): the sample's KL divergence at the returned exposures
    removal_round: np.ndarray  # (N, K) int32: the 0-based trial that removed k, -1 if kept
    kl_increase: np.ndarray  # (N, K): f' - f of the trial that tested k, NaN if never tested
    n_trials: np.ndarray  # (N,) int32
    n_iterations: np.ndarray  # (N,) int64, summed over the solves
    converged: np.ndarray  # (N,) bool: every solve stopped on its tolerance
    dense_exposures: np.ndarray  # (N, K): phase 0, what refit_exposures returns
    dense_errors: np.ndarray  # (N,)
    dense_n_iterations: np.ndarray  # (N,) int32
    dense_converged: np.ndarray  # (N,) bool
    selection_frequency: np.ndarray | None = None  # (N, K): share of the resamples with k in the support
    exposures_quantiles: np.ndarray | None = None  # (Q, N, K)
    exposures_mean: np.ndarray | None = None  # (N, K)
    exposures_resampled: np.ndarray | None = None  # (R, N, K) with keep_resamples
    quantiles: tuple = ()
    max_kl_increase: float = 1.92
    timings: dict = field(default_factory=dict)
    readd_round: np.ndarray | None = None  # (N, K) int32 with readd: the 0-based trial that re-added k, -1 otherwise
    kl_decrease: np.ndarray | None = None  # (N, K) with readd: f - f' of the re-addition trial of k, NaN if never tried
    candidates: np.ndarray | None = None  # (N, K) bool as applied, None = every signature
    required: np.ndarray | None = None  # (N, K) bool as applied, None = none


def check_sets(candidates, required, readd, N: int, K: int):
    """The two masks as ``(N, K)`` bool arrays (or ``None``) and ``readd`` as a bool, or ``ValueError``: each mask is ``None``, a
    boolean array of shape ``(K,)`` for every sample, or one of shape ``(N, K)``; every sample needs a candidate, and a
    required signature must be a candidate."""
    def mask(name, value):
        if value is None:
            return None
        m = np.asarray(value)
        if m.dtype != np.bool_:
            raise ValueError(f"'{name}' must be a boolean array, got dtype {m.dtype}.")
        if m.shape == (K,):
            m = np.broadcast_to(m, (N, K))
        elif m.shape != (N, K):
            raise ValueError(f"'{name}' must have shape ({K},) or ({N}, {K}), got {m.shape}.")
        return np.ascontiguousarray(m)

    if not isinstance(readd, (bool, np.bool_)):
        raise ValueError("'readd' must be True or False.")
    C, Rq = mask("candidates", candidates), mask("required", required)
    if C is not None and not C.any(axis=1).all():
        raise ValueError(f"Sample {int(np.flatnonzero(~C.any(axis=1))[0])} has no candidate signature.")
    if C is not None and Rq is not None and (Rq & ~C).any():
        n, k = np.argwhere(Rq & ~C)[0]
        raise ValueError(f"Sample {int(n)}: required signature {int(k)} is not a candidate.")
    return C, Rq, bool(readd)


def assign_signatures(counts, signatures, max_kl_increase: float = 1.92, n_resamples: int = 0, resample_seed: int = 0,
                      quantiles=(0.025, 0.5, 0.975), min_iterations: int = 500, max_iterations: int = 10000, conv_test_freq: int = 10,
                      tol: float = 1e-7, keep_resamples: bool = False, device: int = 0, chunk_bytes: int | None = None,
                      candidates=None, required=None, readd: bool = False) -> AssignResult:
    """Sparse exposures of every row of ``counts (N, V)`` to the fixed ``signatures (K, V)``, K <= 96 and V <= 96.

    Arguments as :func:`refit_exposures`.  ``max_kl_increase`` is the largest rise of a sample's KL divergence a removal may
    cost; the KL difference is the Poisson log-likelihood difference, so the default 1.92 is half the 95 % point of a
    chi-square with one degree of freedom -- a parameter, not a measurement.  ``max_iterations`` must be a multiple of
    ``conv_test_freq``.  ``candidates`` and ``required`` are ``None`` or boolean masks of shape (K,) or (N, K): the signatures a
    sample may use at all, and those of them that are never tried for removal; they hold for the sample's resamples too.
    ``readd=True`` adds the re-addition pass: removed candidates whose update factor exceeds 1 at the accepted exposures are
    tried again, largest factor first, and kept if the KL divergence falls by more than ``max_kl_increase``.  Anything out of
    range is a ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    X, S, R, seed, min_it, max_it, freq, tol, q, chunk = check_arguments(counts, signatures, n_resamples, resample_seed, quantiles, min_iterations,
                                                                         max_iterations, conv_test_freq, tol, chunk_bytes)
    thr = check_threshold(max_it, freq, max_kl_increase)
    C, Rq, readd = check_sets(candidates, required, readd, X.shape[0], S.shape[0])
    return AssignResult(**call_assign("salnmf_assign_signatures_ex", (), X, S, R, seed, q, min_it, max_it, freq, tol, thr, chunk, C, Rq, readd,
                                      keep_resamples, device, t_start))


def check_threshold(max_iterations: int, conv_test_freq: int, max_kl_increase) -> float:
    """``max_kl_increase`` as a float, or ``ValueError``: a finite number, and ``max_iterations`` a multiple of ``conv_test_freq``."""
    if max_iterations % conv_test_freq != 0:
        raise ValueError("'max_iterations' must be a multiple of 'conv_test_freq': the solves of a sample follow one another on the device.")
    if isinstance(max_kl_increase, bool) or not isinstance(max_kl_increase, (int, float, np.integer, np.floating)) or not np.isfinite(max_kl_increase):
        raise ValueError("'max_kl_increase' must be a finite number.")
    return float(max_kl_increase)


def call_assign(symbol: str, model_args: tuple, X, S, R, seed, q, min_it, max_it, freq, tol, thr, chunk, C, Rq, readd, keep_resamples, device,
                t_start) -> dict:
    """One call of an assignment entry point (``salnmf_assign_signatures_ex``, or ``salnmf_nb_assign_signatures`` with the
    dispersions as ``model_args``, which follow ``n_signatures``) on validated arguments: the fields of :class:`AssignResult`."""
    (N, V), K = X.shape, S.shape[0]
    lib = _lib.load_with_device()
    Q = int(q.size)
    f64 = lambda *shape: np.empty(shape, dtype=np.float64)  # noqa: E731
    i32 = lambda *shape: np.empty(shape, dtype=np.int32)  # noqa: E731
    H, err, kl, Hd, err_d = f64(N, K), f64(N), f64(N, K), f64(N, K), f64(N)
    act, rnd, ntr, conv, nit_d, conv_d = i32(N, K), i32(N, K), i32(N), i32(N), i32(N), i32(N)
    nit = np.empty(N, dtype=np.int64)
    sel = f64(N, K) if R else None
    Hq = f64(Q, N, K) if R else None
    Hm = f64(N, K) if R else None
    Hr = f64(R, N, K) if R and keep_resamples else None
    rrnd = i32(N, K) if readd else None
    kld = f64(N, K) if readd else None
    Cb = None if C is None else C.astype(np.uint8)
    Rb = None if Rq is None else Rq.astype(np.uint8)
    ms = (c_double * 4)()
    p = _lib.pointer
    _lib.check(getattr(lib, symbol)(
        int(device), p(X), N, V, p(S), K, *(p(v) for v in model_args), R, seed, Q if R else 0, p(q), min_it, max_it, freq, tol, thr, chunk, p(Cb),
        p(Rb), int(readd), p(H), p(act), p(err), p(rnd), p(kl), p(ntr), p(nit), p(conv), p(Hd), p(err_d), p(nit_d), p(conv_d), p(sel), p(Hq), p(Hm),
        p(Hr), p(rrnd), p(kld), ctypes.cast(ms, _lib._D),
    ))
    timings = {"resample_s": ms[0] / 1e3, "assign_s": ms[1] / 1e3, "reduce_s": ms[2] / 1e3, "assign_kernel_ms": ms[1],
               "n_chunks": int(ms[3]), "total_s": time.perf_counter() - t_start}
    return dict(exposures=H, active=act.astype(bool), reconstruction_errors=err, removal_round=rnd, kl_increase=kl, n_trials=ntr,
                n_iterations=nit, converged=conv.astype(bool), dense_exposures=Hd, dense_errors=err_d, dense_n_iterations=nit_d,
                dense_converged=conv_d.astype(bool), selection_frequency=sel, exposures_quantiles=Hq, exposures_mean=Hm,
                exposures_resampled=Hr, quantiles=tuple(float(v) for v in q), max_kl_increase=thr, timings=timings, readd_round=rrnd,
                kl_decrease=kld, candidates=C, required=Rq)
