"""Host restatement of the signature-stability contract ("Stability") in NumPy, the assignment by
``scipy.optimize.linear_sum_assignment``.  The yardstick of tests/test_stability_host.py and tests/test_gpu_stability.py.

Besides the results it returns, per solve, the *margin*: the cost of the best assignment that avoids at least one edge of
the optimum (K re-solves, one optimal edge forbidden each) minus the optimal cost.  A test asserts that every margin is far
above rounding, so that no exact solver can come back with another permutation.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np
from scipy.optimize import linear_sum_assignment

FORBIDDEN = 1e6  # (costs are in [0, 2]: an edge of this cost is never taken while another assignment exists)


def assign(D: np.ndarray, margin: bool = True):
    """``p`` minimising ``sum_j D[j, p[j]]`` and its margin (inf for K = 1: there is no other assignment)."""
    rows, cols = linear_sum_assignment(D)
    p = np.empty(len(rows), dtype=np.int32)
    p[rows] = cols
    if not margin:
        return p, np.inf
    best = D[rows, cols].sum()
    second = np.inf
    if len(p) > 1:
        for j in range(len(p)):
            E = D.copy()
            E[j, p[j]] = FORBIDDEN
            r, c = linear_sum_assignment(E)
            second = min(second, E[r, c].sum())
    return p, second - best


def unit_rows(signatures: np.ndarray) -> np.ndarray:
    s = np.asarray(signatures, dtype=np.float64)
    return s / np.sqrt((s * s).sum(axis=2, keepdims=True))


def stability(signatures, errors=None, max_rounds: int = 20, margins: bool = True) -> SimpleNamespace:
    """The contract for one group ``(M, K, V)``; ``margins`` lists the margin of every solve, round after round."""
    u = unit_rows(signatures)
    M, K, V = u.shape
    errors = np.zeros(M) if errors is None else np.asarray(errors, dtype=np.float64)
    anchor = int(np.argmin(errors))  # (the first of equal minima)
    c = u[anchor].copy()
    prev, all_margins = None, []
    converged, n_rounds = False, 0
    for t in range(1, max_rounds + 1):
        p = np.empty((M, K), dtype=np.int32)
        for m in range(M):
            p[m], g = assign(1.0 - c @ u[m].T, margins)
            all_margins.append(g)
        n_rounds = t
        if prev is not None and np.array_equal(p, prev):
            converged = True
            break
        prev = p
        s = np.zeros((K, V))
        for m in range(M):  # members in ascending order
            s += u[m][p[m]]
        if t == max_rounds:
            break
        c = s / np.sqrt((s * s).sum(axis=1, keepdims=True))
    p = prev
    x = np.stack([u[m][p[m]] for m in range(M)])  # (M, K, V): point (m, j)
    xs = np.einsum("mjv,kv->mjk", x, s)  # x . s[j']
    xx = np.einsum("mjv,mjv->mj", x, x)
    own = np.einsum("mjj->mj", xs)
    a = 1.0 - (own - xx) / (M - 1)
    if K == 1:
        b = np.full((M, K), np.nan)
        sil = np.ones((M, K))
    else:
        other = 1.0 - xs / M
        other[:, np.arange(K), np.arange(K)] = np.inf
        b = other.min(axis=2)
        sil = (b - a) / np.maximum(a, b)
    cluster = sil.mean(axis=0)
    return SimpleNamespace(
        assignments=p, n_rounds=n_rounds, converged=converged, consensus=s / s.sum(axis=1, keepdims=True), a=a, b=b, silhouette=sil,
        cluster_stability=cluster, stability_mean=float(cluster.mean()), stability_min=float(cluster.min()),
        margins=np.array(all_margins), points=x, anchor=anchor,
    )


def planted(K: int, M: int, V: int, cv: float, seed: int, mix: float = 0.0):
    """M noisy, row-permuted copies of K Dirichlet signatures (multiplicative gamma noise of coefficient of variation
    ``cv``): ``(signatures (M, K, V), perms (M, K))`` with ``signatures[m, perms[m, j]]`` the copy of signature j.
    ``mix`` > 0 pulls the K signatures towards their mean first: with strong noise the first round, matched against one
    noisy member, then gets some members wrong and later rounds correct them."""
    rng = np.random.default_rng(seed)
    base = rng.dirichlet(np.full(V, 0.2), size=K)
    base = (1.0 - mix) * base + mix * base.mean(axis=0)
    shape = 1.0 / (cv * cv)
    sigs = np.empty((M, K, V))
    perms = np.empty((M, K), dtype=np.int32)
    for m in range(M):
        noisy = base * rng.gamma(shape, 1.0 / shape, size=(K, V))
        noisy /= noisy.sum(axis=1, keepdims=True)
        perms[m] = rng.permutation(K)
        sigs[m, perms[m]] = noisy
    return sigs, perms


def expected_assignments(perms: np.ndarray, anchor: int) -> np.ndarray:
    """The planted assignments as the contract numbers them: cluster j is the signature that row j of the anchor copies."""
    return perms[:, np.argsort(perms[anchor])]


def suggest(ns, mean, low, mean_stability=0.8, min_stability=0.2):
    """The largest K whose mean stability and minimum stability reach the thresholds, or None."""
    ok = [k for k, a, b in zip(ns, mean, low) if a >= mean_stability and b >= min_stability]
    return max(ok) if ok else None
