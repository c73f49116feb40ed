"""Entry-wise comparison on states that sit on the EPSILON clip floor (``tests/test_gpu_floor.py``, ``test_oracle_floor.py``).

A rel-L2 norm cannot see the floor: an entry of 1e-7 next to exposures of 1e3 weighs nothing in it.  The checks here
look at every entry: its relative error against the oracle, whether it sits exactly on the floor wherever the oracle's
value before the clip lies below it, and the NaN / inf pattern.
"""

from __future__ import annotations

import numpy as np

from oracle import klnmf_oracle as orc

EPS = orc.EPSILON


def floor_share(a) -> float:
    """The share of entries exactly at EPSILON."""
    return float(np.mean(np.asarray(a) == EPS))


def lhalf_allowance(t, disc, weights_kl=None, c=8.0):
    """Per-entry absolute allowance of the l-half root ``H = 0.25 t^2 (/ w_kl^2)``, ``t = w_lh/2 - sqrt(disc)``.

    When ``4 H U << w_lh^2`` the subtraction cancels: a rounding of ``sqrt(disc)`` (relative ``eps``) moves ``t`` by
    ``eps sqrt(disc)`` and H by ``0.5 |t| eps sqrt(disc)``.  ``c`` counts the roundings in ``disc`` and ``sqrt``.
    Reference shapes ``(K, N)``; ``weights_kl (N,)``."""
    allow = c * np.finfo(np.float64).eps * np.abs(t) * np.sqrt(disc) / 4.0
    if weights_kl is not None:
        allow = allow / np.asarray(weights_kl) ** 2
    return allow


def assert_entrywise(dev, ref, rtol, pre=None, allowance=None, margin=1e-6, what=""):
    """``dev`` against the oracle's ``ref`` (both clipped, so ``ref >= EPSILON``), entry by entry.

    (a) ``|dev - ref| <= rtol * ref (+ allowance)`` for every finite entry; (b) where the oracle's value before the clip
    ``pre`` lies below ``EPSILON * (1 - margin)``, ``dev`` is exactly EPSILON; (c) the NaN and the inf masks are
    identical.  Returns the largest ``|dev - ref| / ref`` seen (after subtracting the allowance, if any)."""
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), f"{what}: NaN masks differ ({np.isnan(dev).sum()} vs {np.isnan(ref).sum()})"
    assert np.array_equal(np.isinf(dev), np.isinf(ref)), f"{what}: inf masks differ ({np.isinf(dev).sum()} vs {np.isinf(ref).sum()})"
    assert np.array_equal(dev[np.isinf(dev)], ref[np.isinf(ref)]), f"{what}: inf signs differ"
    fin = np.isfinite(ref)
    assert (ref[fin] >= EPS).all(), f"{what}: the reference is not clipped"
    err = np.abs(dev - ref)
    if allowance is not None:
        err = np.maximum(err - np.asarray(allowance), 0.0)
    rel = np.where(fin, err / np.where(fin, ref, 1.0), 0.0)
    worst = float(rel.max()) if rel.size else 0.0
    if worst > rtol:
        i = np.unravel_index(int(np.argmax(rel)), rel.shape)
        raise AssertionError(f"{what}: max relative error {worst:.3e} > {rtol:.1e} at {i}: dev {dev[i]!r} ref {ref[i]!r}")
    if pre is not None:
        below = np.asarray(pre) < EPS * (1.0 - margin)
        off = below & (dev != EPS)
        assert not off.any(), (
            f"{what}: {int(off.sum())} of {int(below.sum())} entries whose oracle value before the clip lies below the floor "
            f"are not exactly EPSILON, e.g. {dev[off][:4]!r}"
        )
    return worst
