"""Count splitting (Poisson thinning) of a count matrix, drawn on the device (``csrc/salnmf_split.h``).

Every single mutation goes to the training matrix with probability ``train_fraction``, independently of all others.  For
Poisson counts of mean lambda the halves ``train`` and ``test = counts - train`` are then independent Poisson counts of means
``p lambda`` and ``(1 - p) lambda``: a model fitted on ``train`` predicts ``test`` with mean ``((1 - p) / p) H W``, and its
KL divergence to ``test`` is an out-of-sample Poisson deviance for every sample and every feature at once.  The draws come
from a counter-based generator (Philox4x32-10), so a call gives the same bits on every run and split f does not depend on
how many are drawn.  ``KLNMFSweep(n_splits=...)`` draws them straight into the batch (``BatchEngine.split``);
:func:`split_counts` is the stand-alone form for any ``n_features <= 3072``.
"""

from __future__ import annotations

import numpy as np

from . import _lib
from .engine import _ptr
from .resample import MAX_FEATURES, _int_in_range, check_counts, check_seed

MAX_SPLITS = 32767


def check_n_splits(n_splits, minimum: int = 1) -> int:
    return _int_in_range(n_splits, minimum, MAX_SPLITS, f"'n_splits' must be an integer in [{minimum}, {MAX_SPLITS}].")


def train_threshold(train_fraction) -> int:
    """``int(p * 2**64)`` for a float ``0 < p < 1``: what crosses the C boundary instead of p.  Scaling a float by a power of
    two is exact, so this is the exact floor of ``p * 2**64``; it must lie in ``[1, 2**64 - 1]``."""
    if not isinstance(train_fraction, (float, np.floating)) or not 0.0 < float(train_fraction) < 1.0:
        raise ValueError("'train_fraction' must be a float with 0 < train_fraction < 1.")
    thr = int(float(train_fraction) * 2.0**64)
    if not 1 <= thr <= 2**64 - 1:
        raise ValueError(f"'train_fraction' = {train_fraction!r} gives the threshold {thr}, outside [1, 2**64 - 1].")
    return thr


def heldout_scale(train_fraction) -> float:
    """``(1 - p) / p``: the factor between the training half's mean and the test half's."""
    p = float(train_fraction)
    return (1.0 - p) / p


def split_counts(counts, n_splits: int = 1, train_fraction: float = 0.5, seed: int = 0, device: int = 0):
    """``n_splits`` count splits of ``counts (N, V)``: ``(train, test)``, each ``(n_splits, N, V)`` float64 of integer
    values with ``train + test == counts``."""
    X = check_counts(counts)
    F, thr, seed = check_n_splits(n_splits), train_threshold(train_fraction), check_seed(seed)
    N, V = X.shape
    if N < 1 or not 1 <= V <= MAX_FEATURES:
        raise ValueError(f"Counts to split need at least one row and 1 to {MAX_FEATURES} columns.")
    lib = _lib.load_with_device()
    train = np.empty((F, N, V), dtype=np.float64)
    test = np.empty((F, N, V), dtype=np.float64)
    _lib.check(lib.salnmf_split_counts(int(device), _ptr(X), N, V, F, thr, seed, _ptr(train), _ptr(test)))
    return train, test
