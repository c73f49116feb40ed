"""Have the exposure shares changed between two samples of one patient?  A calibrated p-value per pair of rows
(``csrc/salnmf_change.h``).

Primary against relapse, before against after treatment, clonal against subclonal mutations: two count vectors of very
different totals, one catalogue.  Two sets of bootstrap quantiles read side by side differ in width with the totals and overlap
whatever the truth; a chi-square test of the raw spectra ignores the catalogue.  :func:`exposure_change_test` fits each sample on
the candidate set C (solves a and b), fits their sum (the pooled solve), and compares "each sample has its own exposures" with
"both have the pooled shares, each its own total": ``statistic = (g_a - f_a) + (g_b - f_b)``, half the likelihood-ratio
statistic.  It then draws ``n_draws`` pairs of count vectors of the two samples' own totals from the pooled fit, puts every pair
through the same procedure, and reports where the observed statistic falls among the null ones:
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
from .refit import _ANNDATA, check_arguments


@dataclass
class ChangeResult:
    statistic: np.ndarray  # (N,): (g_a - f_a) + (g_b - f_b), half the likelihood-ratio statistic; NaN where the pair is untested
    p_value: np.ndarray  # (N,): (1 + n_exceed) / (B + 1); NaN where the pair is untested
    n_exceed: np.ndarray  # (N,) int32: draws b with null_statistics[b, n] >= statistic[n]
    tested: np.ndarray  # (N,) bool: at least two candidates and a positive total on either side
    null_mean: np.ndarray  # (N,): the sum of null_statistics[:, n] in ascending b, divided by B
    exposures_a: np.ndarray  # (N, K): the fit of counts_a on the candidate set (NaN rows where the pair is untested)
    exposures_b: np.ndarray  # (N, K)
    pooled_exposures: np.ndarray  # (N, K): the fit of the two clipped rows' sum
    errors: np.ndarray  # (N, 3): f_a, f_b, f_p
    null_errors: np.ndarray  # (N, 2): g_a, g_b, each sample's divergence from its share of the pooled spectrum
    n_iterations: np.ndarray  # (N, 3) int32: the observed solves a, b, pooled
    converged: np.ndarray  # (N, 3) bool
    shares_a: np.ndarray  # (N, K): exposures_a / its row sums
    shares_b: np.ndarray  # (N, K)
    share_difference: np.ndarray  # (N, K): shares_b - shares_a
    null_statistics: np.ndarray  # (B, N)
    null_n_iterations: np.ndarray  # (B, N, 3) int32
    candidates: np.ndarray | None = None  # (N, K) bool as applied, None = every signature
    draws: np.ndarray | None = None  # (B, N, 2, V) with keep_draws
    timings: dict = field(default_factory=dict)


def check_change_arguments(counts_a, counts_b, signatures, n_draws, seed, candidates, min_iterations, max_iterations, conv_test_freq, tol, chunk_bytes):
    """What :func:`exposure_change_test` checks before it touches a device ->
    ``(Xa, Xb, W, C, B, seed, min_it, max_it, freq, tol, chunk)``."""
    Xa, W, _, seed, min_it, max_it, freq, tol, _, chunk = check_arguments(counts_a, signatures, 0, seed, (), min_iterations, max_iterations,
                                                                         conv_test_freq, tol, chunk_bytes)
    shape_b = np.shape(counts_b.X if isinstance(counts_b, _ANNDATA) else counts_b)
    if shape_b != Xa.shape:
        raise ValueError(f"Row n of 'counts_a' and row n of 'counts_b' form pair n: the shapes must agree, got {Xa.shape} and {shape_b}.")
    Xb = check_arguments(counts_b, W, 0, seed, (), min_it, max_it, freq, tol, chunk)[0]
    if max_it % freq != 0:
        raise ValueError("'max_iterations' must be a multiple of 'conv_test_freq': the three solves of a pair follow one another on the device.")
    for name, X in (("counts_a", Xa), ("counts_b", Xb)):
        try:
            check_integer_counts(X)
        except ValueError as err:
            raise ValueError(f"'{name}': {err}") from None
    B = check_n_draws(n_draws)
    C, _, _ = check_sets(candidates, None, False, Xa.shape[0], W.shape[0])
    return Xa, Xb, W, C, B, seed, min_it, max_it, freq, tol, chunk


def shares(exposures: np.ndarray) -> np.ndarray:
    """Rows of exposures divided by their sums (NaN rows stay NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return exposures / exposures.sum(axis=1, keepdims=True)


class ChangeOutputs:
    """The arrays ``salnmf_exposure_change`` fills, in the C order, and the :class:`ChangeResult` made of them."""

    def __init__(self, N, V, K, B, keep_draws):
        f64 = lambda *shape: np.empty(shape, dtype=np.float64)  # noqa: E731
        i32 = lambda *shape: np.empty(shape, dtype=np.int32)  # noqa: E731
        self.B = B
        self.tested = np.zeros(N, dtype=np.uint8)
        self.stat, self.mean = np.full(N, np.nan), np.full(N, np.nan)
        self.Ha, self.Hb, self.H0 = np.full((N, K), np.nan), np.full((N, K), np.nan), np.full((N, K), np.nan)
        self.err, self.err0 = f64(N, 3), f64(N, 2)
        self.exceed, self.nit, self.conv = i32(N), i32(N, 3), i32(N, 3)
        self.stat_b, self.nit_b = f64(B, N), i32(B, N, 3)
        self.drawn = f64(B, N, 2, V) if keep_draws else None

    def pointers(self):
        p = _lib.pointer
        return (p(self.tested), p(self.stat), p(self.exceed), p(self.mean), p(self.Ha), p(self.Hb), p(self.H0), p(self.err), p(self.err0),
                p(self.nit), p(self.conv), p(self.stat_b), p(self.nit_b), p(self.drawn))

    def result(self, C, ms, total_s) -> ChangeResult:
        tested = self.tested.astype(bool)
        timings = {"draw_s": ms[0] / 1e3, "solve_s": ms[1] / 1e3, "reduce_s": ms[2] / 1e3, "change_kernel_ms": ms[1], "n_chunks": int(ms[3]),
                   "total_s": total_s}
        p_value = np.where(tested, (1 + self.exceed.astype(np.int64)) / (self.B + 1), np.nan)
        shares_a, shares_b = shares(self.Ha), shares(self.Hb)
        return ChangeResult(statistic=self.stat, p_value=p_value, n_exceed=self.exceed, tested=tested, null_mean=self.mean, exposures_a=self.Ha,
                            exposures_b=self.Hb, pooled_exposures=self.H0, errors=self.err, null_errors=self.err0, n_iterations=self.nit,
                            converged=self.conv.astype(bool), shares_a=shares_a, shares_b=shares_b, share_difference=shares_b - shares_a,
                            null_statistics=self.stat_b, null_n_iterations=self.nit_b, candidates=C, draws=self.drawn, timings=timings)


def exposure_change_test(counts_a, counts_b, signatures, n_draws: int = 200, seed: int = 0, candidates=None, min_iterations: int = 500,
                         max_iterations: int = 10000, conv_test_freq: int = 10, tol: float = 1e-7, keep_draws: bool = False,
                         chunk_bytes: int | None = None, device: int = 0) -> ChangeResult:
    """The bootstrap likelihood-ratio test of "the same exposure shares" for every pair (row n of ``counts_a``, row n of
    ``counts_b``), both (N, V), against the fixed ``signatures (K, V)``, K <= 96 and V <= 96.

    With C the pair's candidate set (``candidates``: ``None``, or a boolean mask of shape (K,) or (N, K), as
    :func:`assign_signatures` takes it; it holds for both samples and for the pooled fit): the three observed fits are
    ``assign_signatures(x, signatures, candidates=C, required=C, ...)`` of row a, of row b and of the sum of the two clipped
    rows, bit for bit with the same iteration arguments.  ``null_errors`` are the two samples' divergences from their shares
    ``t / (t_a + t_b)`` of the pooled spectrum, and ``statistic = (g_a - f_a) + (g_b - f_b)``.  Null draw b is a pair of count
    vectors of the two samples' own totals drawn from the pooled fit, and goes through the same three solves.  A pair with fewer
    than two candidates or an empty row is untested: NaN, ``tested`` False, no draw and no solve.

    ``p_value`` is per pair, conditional on both totals, drawn from a fitted model, uncorrected for multiplicity and never below
    ``1 / (n_draws + 1)``.  It says *that* the shares differ, not *which* signature's: ``share_difference`` is descriptive, and
    :func:`exposure_intervals` on each sample gives the per-signature uncertainty.  ``max_iterations`` must be a multiple of
    ``conv_test_freq``; ``chunk_bytes`` bounds the device buffer the draws are written into (default 256 MiB; the result does
    not depend on it).  The counts are non-negative integers with row totals below 2**32; anything out of range is a
    ``ValueError`` before the device is touched."""
    t_start = time.perf_counter()
    Xa, Xb, W, C, B, seed, min_it, max_it, freq, tol, chunk = check_change_arguments(counts_a, counts_b, signatures, n_draws, seed, candidates,
                                                                                     min_iterations, max_iterations, conv_test_freq, tol, chunk_bytes)
    (N, V), K = Xa.shape, W.shape[0]
    if not isinstance(keep_draws, (bool, np.bool_)):
        raise ValueError("'keep_draws' must be True or False.")
    lib = _lib.load_with_device()
    out = ChangeOutputs(N, V, K, B, bool(keep_draws))
    Cb = None if C is None else C.astype(np.uint8)
    ms = (c_double * 4)()
    p = _lib.pointer
    _lib.check(lib.salnmf_exposure_change(
        int(device), p(Xa), N, V, p(Xb), N, V, p(W), K, p(Cb), B, seed, min_it, max_it, freq, tol, chunk, *out.pointers(), ctypes.cast(ms, _lib._D),
    ))
    return out.result(C, ms, time.perf_counter() - t_start)
