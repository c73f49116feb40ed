"""Stability of signatures across many fits, matched and scored on the device (``csrc/salnmf_stability.h``, DESIGN.md
section 12, "Stability").

A *group* is M >= 2 signature matrices of one shape ``(K, V)``, K <= 16, V <= 96 -- the fits of one K over seeds and
bootstrap resamples -- and one error value per member.  The rows are scaled to unit Euclidean norm, the member of smallest
error provides the first centroids, and each round assigns every member's rows to the centroids by the optimal assignment
under the cost ``1 - cosine``, sums each cluster over the members and, unless no assignment changed, takes the normalised
sums as the next centroids.  The silhouettes under the cosine distance follow from the cluster sums.
``KLNMFSweep(stability=True)`` runs this on the signatures where the sweep left them (``BatchEngine.stability``);
:func:`signature_stability` is the stand-alone form for signatures held on the host.
"""

from __future__ import annotations

import ctypes
from ctypes import c_double
from dataclasses import dataclass

import numpy as np

from . import _lib
from .engine import _ptr

MAX_SIGNATURES = 16
MAX_FEATURES = 96


@dataclass
class StabilityResult:
    """What the matching of one group gives.  Point (m, j) is the row of member m assigned to cluster j."""

    assignments: np.ndarray  # (M, K) int32: the row of member m in cluster j
    n_rounds: int
    converged: bool
    consensus: np.ndarray  # (K, V): the cluster sums, rows scaled to sum one
    a: np.ndarray  # (M, K): mean cosine distance of a point to the rest of its cluster
    b: np.ndarray  # (M, K): its smallest mean distance to another cluster (NaN for K = 1)
    silhouette: np.ndarray  # (M, K): (b - a) / max(a, b); 1 for K = 1
    cluster_stability: np.ndarray  # (K,): mean silhouette of a cluster over the members
    stability_mean: float
    stability_min: float
    kernel_ms: float = 0.0  # the launch (all groups of the call) by device events


def check_max_rounds(max_rounds) -> int:
    if not isinstance(max_rounds, (int, np.integer)) or isinstance(max_rounds, bool) or int(max_rounds) < 1:
        raise ValueError("'max_rounds' must be a positive integer.")
    return int(max_rounds)


def check_group_shape(M: int, K: int, V: int) -> None:
    if not 1 <= K <= MAX_SIGNATURES:
        raise ValueError(f"Signature stability handles 1 to {MAX_SIGNATURES} signatures per member, got {K}.")
    if not 1 <= V <= MAX_FEATURES:
        raise ValueError(f"Signature stability handles 1 to {MAX_FEATURES} features, got {V}.")
    if M < 2:
        raise ValueError(f"A group needs at least 2 members, got {M}.")


class _Outputs:
    """The padded output arrays of one launch over groups of ``(M, K)`` members and their pointers in the C ABI's order."""

    def __init__(self, shapes):
        self.shapes = list(shapes)
        T, G = sum(m for m, _ in self.shapes), len(self.shapes)
        self.assignments = np.empty((T, MAX_SIGNATURES), dtype=np.int32)
        self.n_rounds = np.empty(G, dtype=np.int32)
        self.converged = np.empty(G, dtype=np.int32)
        self.consensus = np.empty((G, MAX_SIGNATURES, MAX_FEATURES), dtype=np.float64)
        self.a = np.empty((T, MAX_SIGNATURES), dtype=np.float64)
        self.b = np.empty((T, MAX_SIGNATURES), dtype=np.float64)
        self.silhouette = np.empty((T, MAX_SIGNATURES), dtype=np.float64)
        self.cluster = np.empty((G, MAX_SIGNATURES), dtype=np.float64)
        self.score = np.empty((G, 2), dtype=np.float64)
        self.kernel_ms = c_double(0.0)

    def pointers(self):
        ints = [a.ctypes.data_as(_lib._I) for a in (self.assignments, self.n_rounds, self.converged)]
        return (*ints, *[_ptr(a) for a in (self.consensus, self.a, self.b, self.silhouette, self.cluster, self.score)],
                ctypes.cast(ctypes.byref(self.kernel_ms), _lib._D))

    def results(self, V: int) -> list[StabilityResult]:
        out, first = [], 0
        for g, (M, K) in enumerate(self.shapes):
            rows = slice(first, first + M)
            out.append(StabilityResult(
                assignments=self.assignments[rows, :K].copy(), n_rounds=int(self.n_rounds[g]), converged=bool(self.converged[g]),
                consensus=self.consensus[g, :K, :V].copy(), a=self.a[rows, :K].copy(), b=self.b[rows, :K].copy(),
                silhouette=self.silhouette[rows, :K].copy(), cluster_stability=self.cluster[g, :K].copy(),
                stability_mean=float(self.score[g, 0]), stability_min=float(self.score[g, 1]), kernel_ms=float(self.kernel_ms.value),
            ))
            first += M
        return out


def check_errors(errors, shapes, single: bool = False) -> np.ndarray | None:
    """One error per member of every group (``single``: of the one group), concatenated in group order; None stays None
    (all zero)."""
    if errors is None:
        return None
    per_group = [errors] if single else list(errors)
    if len(per_group) != len(shapes):
        raise ValueError("'errors' must hold one sequence per group.")
    flat = []
    for e, (M, _) in zip(per_group, shapes):
        e = np.asarray(e, dtype=np.float64).reshape(-1)
        if e.shape != (M,):
            raise ValueError(f"'errors' must hold one value per member: expected {M}, got {e.size}.")
        if np.isnan(e).any():
            raise ValueError("'errors' must not hold NaNs.")
        flat.append(e)
    return np.ascontiguousarray(np.concatenate(flat))


def signature_stability(signatures, errors=None, max_rounds: int = 20, device: int = 0):
    """Match, cluster and score the signatures of M fits.

    ``signatures`` is one ``(M, K, V)`` array, or a list of such arrays of one V (one group each, all in one launch);
    ``errors`` one value per member (a list of sequences for a list of groups), the smallest naming the member that
    provides the first centroids.  Returns one :class:`StabilityResult`, or a list of them for a list.  ``ValueError`` for
    K > 16, V > 96, M < 2 and for a signature that is not finite or is all zero."""
    single = isinstance(signatures, np.ndarray) and signatures.ndim == 3
    groups = [np.ascontiguousarray(s, dtype=np.float64) for s in ([signatures] if single else signatures)]
    max_rounds = check_max_rounds(max_rounds)
    if not groups:
        raise ValueError("'signatures' must hold at least one group.")
    for s in groups:
        if s.ndim != 3:
            raise ValueError("Every group of signatures must be an array (members, signatures, features).")
        check_group_shape(*s.shape)
        if s.shape[2] != groups[0].shape[2]:
            raise ValueError("All groups must have the same number of features.")
        norms = np.sqrt((s * s).sum(axis=2))
        if not np.isfinite(s).all() or not np.isfinite(norms).all() or (norms <= 0).any():
            raise ValueError("Every signature needs finite entries and a positive norm.")
    shapes = [(s.shape[0], s.shape[1]) for s in groups]
    V = groups[0].shape[2]
    errs = check_errors(errors, shapes, single)
    lib = _lib.load()
    if lib.salnmf_device_count() < 1:
        raise _lib.EngineUnavailable("no HIP device visible: salamander_amd runs on MI355X (gfx950) only and has no CPU fallback.")
    padded = np.zeros((sum(m for m, _ in shapes), MAX_SIGNATURES, MAX_FEATURES), dtype=np.float64)
    first = 0
    for s in groups:
        padded[first : first + s.shape[0], : s.shape[1], :V] = s
        first += s.shape[0]
    out = _Outputs(shapes)
    ks = np.ascontiguousarray([k for _, k in shapes], dtype=np.int32)
    ms = np.ascontiguousarray([m for m, _ in shapes], dtype=np.int32)
    _lib.check(lib.salnmf_signature_stability(
        int(device), _ptr(padded), len(shapes), ks.ctypes.data_as(_lib._I), ms.ctypes.data_as(_lib._I), V,
        None if errs is None else _ptr(errs), max_rounds, *out.pointers(),
    ))
    results = out.results(V)
    return results[0] if single else results
