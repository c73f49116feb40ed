"""A NumPy replica of the device's count splitting (``csrc/salnmf_split.h``) -- TESTS ONLY.

Written from the contract, not from the kernel: ``thr = int(p * 2**64)``; mutation j of row n (``0 <= j < T_n``) belongs to
cell ``v(j)``, the smallest v with ``cum[v] > j``; Philox4x32-10 with key ``(seed & 0xffffffff, seed >> 32)``; block q of
row n of split f has counter ``(q, 0x53504C54, n, f)``; draw 2q uses ``u = o0 | o1 << 32``, draw 2q + 1 uses
``u = o2 | o3 << 32``, draws ``j >= T_n`` are discarded; mutation j goes to train iff ``u_j < thr``.  ``train[n, v]`` counts
the mutations of cell v sent to train and ``test = X - train``."""

import numpy as np

from _resample_ref import MASK, S32, check, philox4x32_10

STREAM = 0x53504C54


def threshold(p):
    """``int(p * 2**64)`` for a float 0 < p < 1, in [1, 2**64 - 1]."""
    assert isinstance(p, float) and 0.0 < p < 1.0
    thr = int(p * 2.0**64)
    assert 1 <= thr <= 2**64 - 1
    return thr


def draws(T, n, f, seed):
    """The T 64-bit draws of row n of split f, as Python-exact uint64."""
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    q = np.arange((T + 1) // 2, dtype=np.uint64)
    o0, o1, o2, o3 = philox4x32_10(q & MASK, np.full_like(q, STREAM), np.full_like(q, n), np.full_like(q, f), k0, k1)
    u = np.stack([o0 | (o1 << S32), o2 | (o3 << S32)], axis=1).reshape(-1)  # draws 2q, 2q + 1
    return u[:T]


def split_row(row, n, f, seed, thr):
    """One row of one split: ``row`` uint64 counts -> int64 train counts."""
    V = len(row)
    T = int(row.sum())
    to_train = draws(T, n, f, seed) < np.uint64(thr)
    cell = np.repeat(np.arange(V), row.astype(np.int64))  # cell of mutation j: the smallest v with cum[v] > j
    return np.bincount(cell[to_train], minlength=V).astype(np.int64)


def split_counts(X, n_splits, train_fraction=0.5, seed=0):
    """``(train, test)``, each ``(n_splits, N, V)`` float64 of integer values: what ``sal.split_counts`` must return."""
    Xi = check(X)
    seed = int(seed)
    assert 0 <= seed < 2**64
    thr = threshold(train_fraction)
    N, V = Xi.shape
    train = np.zeros((n_splits, N, V), dtype=np.float64)
    for f in range(n_splits):
        for n in range(N):
            train[f, n] = split_row(Xi[n], n, f, seed, thr)
    return train, Xi.astype(np.float64)[None] - train
