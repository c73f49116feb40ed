"""Bootstrap resamples of a count matrix, drawn on the device (``csrc/salnmf_resample.h``).

Row n of every resample is one multinomial draw of the row's own total from its own observed spectrum -- each sample's
mutations redrawn -- by a counter-based generator (Philox4x32-10), so a call gives the same bits on every run and resample
r does not depend on how many are drawn.  ``KLNMFSweep(n_resamples=...)`` draws them straight into the batch
(``BatchEngine.resample``); :func:`resample_counts` is the stand-alone form for any ``n_features <= 3072``.
"""

from __future__ import annotations

import numpy as np

from . import _lib
from .engine import _ptr

MAX_RESAMPLES = 65535
MAX_FEATURES = 3072


def _int_in_range(value, low: int, high: int, message: str) -> int:
    """``int(value)`` for an integer (no bool) with ``low <= value <= high``, else ``ValueError(message)``."""
    if not isinstance(value, (int, np.integer)) or isinstance(value, bool) or not low <= int(value) <= high:
        raise ValueError(message)
    return int(value)


def check_seed(seed) -> int:
    return _int_in_range(seed, 0, 2**64 - 1, "'seed' of a resample must be an integer in [0, 2**64).")


def check_n_resamples(n_resamples, minimum: int = 1) -> int:
    return _int_in_range(n_resamples, minimum, MAX_RESAMPLES, f"'n_resamples' must be an integer in [{minimum}, {MAX_RESAMPLES}].")


def check_counts(X) -> np.ndarray:
    """``X`` as a C-ordered float64 matrix, or ``ValueError`` naming the first row a resample cannot be drawn from: an
    entry that is negative or not an integer value, or a row total of 2**32 or more."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("Counts to resample must be a matrix (samples x features).")
    bad = ~((X >= 0) & (X == np.floor(X)) & np.isfinite(X))
    rows = np.flatnonzero(bad.any(axis=1))
    if rows.size:
        n = int(rows[0])
        v = int(np.flatnonzero(bad[n])[0])
        raise ValueError(f"Resampling needs non-negative integer counts: row {n}, column {v} holds {X[n, v]!r}.")
    rows = np.flatnonzero(X.sum(axis=1) >= 2.0**32)
    if rows.size:
        raise ValueError(f"Resampling needs row totals below 2**32: row {int(rows[0])} sums to {X[int(rows[0])].sum():.0f}.")
    return X


def resample_counts(X, n_resamples: int, seed: int = 0, device: int = 0) -> np.ndarray:
    """``n_resamples`` bootstrap resamples of the counts ``X (N, V)``: ``(n_resamples, N, V)`` float64 of integer values."""
    X = check_counts(X)
    R, seed = check_n_resamples(n_resamples), check_seed(seed)
    N, V = X.shape
    if N < 1 or not 1 <= V <= MAX_FEATURES:
        raise ValueError(f"Counts to resample need at least one row and 1 to {MAX_FEATURES} columns.")
    lib = _lib.load_with_device()
    out = np.empty((R, N, V), dtype=np.float64)
    _lib.check(lib.salnmf_resample_counts(int(device), _ptr(X), N, V, R, seed, _ptr(out)))
    return out
