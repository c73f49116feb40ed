"""A NumPy replica of the device's bootstrap resampler (``csrc/salnmf_resample.h``) -- TESTS ONLY.

Written from the contract, not from the kernel: Philox4x32-10 with key ``(seed & 0xffffffff, seed >> 32)``; block q of row
n of resample r has counter ``(q mod 2**32, q >> 32, n, r)``; draw 2q uses ``u = o0 | o1 << 32``, draw 2q + 1 uses
``u = o2 | o3 << 32``; ``t = floor(u T / 2**64)``; the draw lands in the smallest v with ``cum[v] > t``.  All in uint64:
with T < 2**32, ``t = (uhi T + ((ulo T) >> 32)) >> 32`` never overflows."""

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays of 32-bit words held in uint64; returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def check(X):
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim == 2 and (X >= 0).all() and (X == np.floor(X)).all(), "integer counts only"
    Xi = X.astype(np.uint64)
    assert (Xi.sum(axis=1) < 2**32).all(), "row totals below 2**32"
    return Xi


def resample_row(row, n, r, seed, chunk=1 << 20):
    """One row of one resample: ``row`` uint64 counts -> int64 counts."""
    V = len(row)
    cum = np.cumsum(row, dtype=np.uint64)
    T = int(cum[-1])
    out = np.zeros(V, dtype=np.int64)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    n_blocks = (T + 1) // 2
    Tu = np.uint64(T)
    for start in range(0, n_blocks, chunk):
        q = np.arange(start, min(start + chunk, n_blocks), dtype=np.uint64)
        o0, o1, o2, o3 = philox4x32_10(q & MASK, q >> S32, np.full_like(q, n), np.full_like(q, r), k0, k1)
        ulo = np.stack([o0, o2], axis=1).reshape(-1)  # draws 2q, 2q + 1
        uhi = np.stack([o1, o3], axis=1).reshape(-1)
        keep = 2 * int(q[0]) + np.arange(len(ulo)) < T
        ulo, uhi = ulo[keep], uhi[keep]
        t = (uhi * Tu + ((ulo * Tu) >> S32)) >> S32
        out += np.bincount(np.searchsorted(cum, t, side="right"), minlength=V)
    return out


def resample_counts(X, n_resamples, seed=0):
    """``(n_resamples, N, V)`` float64 of integer values: what ``sal.resample_counts`` must return, entry for entry."""
    Xi = check(X)
    seed = int(seed)
    assert 0 <= seed < 2**64
    N, V = Xi.shape
    out = np.zeros((n_resamples, N, V), dtype=np.float64)
    for r in range(n_resamples):
        for n in range(N):
            out[r, n] = resample_row(Xi[n], n, r, seed)
    return out
