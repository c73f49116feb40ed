"""Which signature's share has changed between two samples of one patient?  A calibrated p-value per (pair of rows, tested
signature) (``csrc/salnmf_sigchange.h``).

:func:`exposure_change_test` says *that* the shares of a pair differ.  :func:`signature_change_test` asks the next question, one
signature at a time: did the platinum signature appear at relapse, did APOBEC grow in the subclone?  The share of signature s in
a sample is ``h_s / t``, its exposure over the sample's total.  For every pair and every tested s it fits each sample on the
candidate set C (solves a and b), fits both samples side by side with the share of s tied and everything else free (the tied
solve), and compares the two: ``statistic = (f_a0 - f_a) + (f_b0 - f_b)``, half the likelihood-ratio statistic with one
constrained parameter.  It then draws ``n_draws`` pairs of count vectors of the two samples' own totals from the tied fit, puts
every pair through the same three solves, and reports where the observed statistic falls among the null ones:
``p_value = (1 + n_exceed) / (n_draws + 1)``.  Everything runs on the device; there is no CPU fallback.
"""

from __future__ import annotations

import ctypes
import time
from ctypes import c_double
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .change import check_change_arguments
from .presence import check_test
from .utils import EPSILON


@dataclass
class SignatureChangeResult:
    statistic: np.ndarray  # (N, S): (f_a0 - f_a) + (f_b0 - f_b), half the likelihood-ratio statistic; NaN where untested
    p_value: np.ndarray  # (N, S): (1 + n_exceed) / (B + 1); NaN where untested
    n_exceed: np.ndarray  # (N, S) int32: draws b with null_statistics[b, n, j] >= statistic[n, j]
    tested: np.ndarray  # (N, S) bool: s is a candidate and not the only one, and both rows have a positive total
    null_mean: np.ndarray  # (N, S): the sum of null_statistics[:, n, j] in ascending b, divided by B
    share_a: np.ndarray  # (N, S): exposures_a[n, s] / t_a, t the sum of the clipped row
    share_b: np.ndarray  # (N, S)
    share_difference: np.ndarray  # (N, S): share_b - share_a
    tied_share: np.ndarray  # (N, S): (h_as0 + h_bs0) / (t_a + t_b), the common share of the tied fit
    exposures_a: np.ndarray  # (N, K): the fit of counts_a on the candidate set (NaN rows where no problem of the pair is tested)
    exposures_b: np.ndarray  # (N, K)
    tied_exposures_a: np.ndarray  # (N, S, K): sample a's exposures in the tied fit of signature s
    tied_exposures_b: np.ndarray  # (N, S, K)
    errors: np.ndarray  # (N, S, 4): f_a, f_b, f_a0, f_b0
    n_iterations: np.ndarray  # (N, S, 3) int32: the observed solves a, b, tied
    converged: np.ndarray  # (N, S, 3) bool
    null_statistics: np.ndarray  # (B, N, S)
    null_n_iterations: np.ndarray  # (B, N, S, 3) int32
    test: tuple = ()
    candidates: np.ndarray | None = None  # (N, K) bool as applied, None = every signature
    draws: np.ndarray | None = None  # (B, N, S, 2, V) with keep_draws
    timings: dict = field(default_factory=dict)


def check_signature_change_arguments(counts_a, counts_b, signatures, test, n_draws, seed, candidates, min_iterations, max_iterations,
                                     conv_test_freq, tol, chunk_bytes):
    """What :func:`signature_change_test` checks before it touches a device ->
    ``(Xa, Xb, W, T, C, B, seed, min_it, max_it, freq, tol, chunk)``."""
    Xa, Xb, W, C, B, seed, min_it, max_it, freq, tol, chunk = check_change_arguments(counts_a, counts_b, signatures, n_draws, seed, candidates,
                                                                                     min_iterations, max_iterations, conv_test_freq, tol, chunk_bytes)
    T = check_test(test, W.shape[0])
    return Xa, Xb, W, T, C, B, seed, min_it, max_it, freq, tol, chunk


def clipped_totals(X: np.ndarray) -> np.ndarray:
    """The sums of the rows clipped to EPSILON: the t of a share h_s / t."""
    return np.maximum(X, EPSILON).sum(axis=1)


class SignatureChangeOutputs:
    """The arrays ``salnmf_signature_change`` fills, in the C order, and the :class:`SignatureChangeResult` made of them."""

    def __init__(self, N, V, K, S, B, keep_draws):
        f64 = lambda *shape: np.empty(shape, dtype=np.float64)  # noqa: E731
        i32 = lambda *shape: np.empty(shape, dtype=np.int32)  # noqa: E731
        self.B = B
        self.tested = np.zeros((N, S), dtype=np.uint8)
        self.stat, self.mean = np.full((N, S), np.nan), np.full((N, S), np.nan)
        self.Ha, self.Hb = np.full((N, K), np.nan), np.full((N, K), np.nan)
        self.Ha0, self.Hb0 = np.full((N, S, K), np.nan), np.full((N, S, K), np.nan)
        self.err = np.full((N, S, 4), np.nan)
        self.exceed, self.nit, self.conv = i32(N, S), i32(N, S, 3), i32(N, S, 3)
        self.stat_b, self.nit_b = f64(B, N, S), i32(B, N, S, 3)
        self.drawn = f64(B, N, S, 2, V) if keep_draws else None

    def pointers(self):
        p = _lib.pointer
        return (p(self.tested), p(self.stat), p(self.exceed), p(self.mean), p(self.Ha), p(self.Hb), p(self.Ha0), p(self.Hb0), p(self.err),
                p(self.nit), p(self.conv), p(self.stat_b), p(self.nit_b), p(self.drawn))

    def result(self, T, C, Xa, Xb, ms, total_s) -> SignatureChangeResult:
        tested = self.tested.astype(bool)
        timings = {"draw_s": ms[0] / 1e3, "solve_s": ms[1] / 1e3, "reduce_s": ms[2] / 1e3, "sigchange_kernel_ms": ms[1], "n_chunks": int(ms[3]),
                   "total_s": total_s}
        p_value = np.where(tested, (1 + self.exceed.astype(np.int64)) / (self.B + 1), np.nan)
        ta, tb = clipped_totals(Xa)[:, None], clipped_totals(Xb)[:, None]
        idx = np.asarray(T, dtype=np.int64)
        rows = np.arange(tested.shape[0])[:, None], np.arange(idx.size)[None, :], idx[None, :]
        share_a = np.where(tested, self.Ha[:, idx] / ta, np.nan)
        share_b = np.where(tested, self.Hb[:, idx] / tb, np.nan)
        tied_share = (self.Ha0[rows] + self.Hb0[rows]) / (ta + tb)
        return SignatureChangeResult(statistic=self.stat, p_value=p_value, n_exceed=self.exceed, tested=tested, null_mean=self.mean, share_a=share_a,
                                     share_b=share_b, share_difference=share_b - share_a, tied_share=tied_share, exposures_a=self.Ha,
                                     exposures_b=self.Hb, tied_exposures_a=self.Ha0, tied_exposures_b=self.Hb0, errors=self.err,
                                     n_iterations=self.nit, converged=self.conv.astype(bool), null_statistics=self.stat_b,
                                     null_n_iterations=self.nit_b, test=tuple(int(v) for v in T), candidates=C, draws=self.drawn, timings=timings)


def signature_change_test(counts_a, counts_b, signatures, test, n_draws: int = 200, seed: int = 0, candidates=None, min_iterations: int = 500,
                          max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7, keep_draws: bool = False,
                          chunk_bytes: int | None = None, device: int = 0) -> SignatureChangeResult:
    """The bootstrap likelihood-ratio test of "signature s has the same share in both samples" for every pair (row n of
    ``counts_a``, row n of ``counts_b``), both (N, V), and every s in ``test``, against the fixed ``signatures (K, V)``, K <= 96 and
    V <= 96.

    With C the pair's candidate set (``candidates``: ``None``, or a boolean mask of shape (K,) or (N, K), as
    :func:`assign_signatures` takes it; it holds for both samples) and s = ``test[j]``: the two free fits are
    ``assign_signatures(x, signatures, candidates=C, required=C, ...)`` of row a and of row b, bit for bit with the same iteration
    arguments.  The tied fit runs both samples side by side from the cold start: every exposure but s takes its own sample's
    update factor, s takes ``c_a u_as + c_b u_bs`` in both, ``c = t / (t_a + t_b)``, so that ``h_as / t_a = h_bs / t_b`` wherever
    neither sits at the EPSILON floor; it stops on ``f_a0 + f_b0``.  ``statistic[n, j] = (f_a0 - f_a) + (f_b0 - f_b)``.  Null draw b
    is a pair of count vectors of the two samples' own totals, each drawn from its own side of the tied fit, and goes through
    the same three solves.  A problem with s outside C, fewer than two candidates or an empty row is untested: NaN, ``tested``
    False, no draw and no solve.  Exchanging ``counts_a`` and ``counts_b`` exchanges the sides and leaves the statistic's bits, and a
    pair whose two samples have the same update factor of s at every step (``counts_b = m * counts_a``) has statistic 0.0.

    ``p_value`` is per pair and per signature, conditional on both totals, drawn from a fitted model, uncorrected for
    multiplicity across signatures and pairs, never below ``1 / (n_draws + 1)``, and conservative where s sits at the floor in
    both samples.  ``max_iterations`` must be a multiple of ``conv_test_freq``; ``chunk_bytes`` bounds the device buffer the draws
    are written into (default 256 MiB; the result does not depend on it).  The counts are non-negative integers with row totals
    below 2**32; anything out of range is a ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    Xa, Xb, W, T, C, B, seed, min_it, max_it, freq, tol, chunk = check_signature_change_arguments(
        counts_a, counts_b, signatures, test, n_draws, seed, candidates, min_iterations, max_iterations, conv_test_freq, tol, chunk_bytes)
    (N, V), K, S = Xa.shape, W.shape[0], int(T.size)
    if not isinstance(keep_draws, (bool, np.bool_)):
        raise ValueError("'keep_draws' must be True or False.")
    lib = _lib.load_with_device()
    out = SignatureChangeOutputs(N, V, K, S, B, bool(keep_draws))
    Cb = None if C is None else C.astype(np.uint8)
    ms = (c_double * 4)()
    p = _lib.pointer
    _lib.check(lib.salnmf_signature_change(
        int(device), p(Xa), N, V, p(Xb), N, V, p(W), K, p(T), S, p(Cb), B, seed, min_it, max_it, freq, tol, chunk, *out.pointers(),
        ctypes.cast(ms, _lib._D),
    ))
    return out.result(T, C, Xa, Xb, ms, time.perf_counter() - t_start)
