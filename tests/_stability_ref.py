"""Host restatement of the signature-stability contract ("Stability") in NumPy, the assignment by
``scipy.optimize.linear_sum_assignment``.  The yardstick of tests/test_stability_host.py and tests/test_gpu_stability.py.

Besides the results it returns, per solve, the *margin*: the cost of the best assignment that avoids at least one edge of
the optimum (K re-solves, one optimal edge forbidden each) minus the optimal cost.  A test asserts that every margin is far
above rounding, so that no exact solver can come back with another permutation.

Further down: the device's own assignment solve restated lane by lane (``lane_assign``), a plain Hungarian solve that counts
the columns of every augmenting path, and seeded generators of groups whose first round solves a prescribed cost tile
(``block_group`` and the families built on it) -- the inputs of tests/test_stability_solver_host.py and of the constructed
cases of tests/test_gpu_stability.py.
"""

from __future__ import annotations

import functools
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
        margins=np.array(all_margins), points=x, anchor=anchor, centroids=c, unit=u,
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


# ------------------------------------------------------------------ the device's assignment solve, lane by lane
KINF = 1e300  # (stab_assign's kInf)
LANES = 16


def lane_assign(D, K: int) -> np.ndarray:
    """``stab_assign`` of csrc/salnmf_stability.h line by line: the 16 lane states of a row of lanes as arrays of length
    16 (with a leading axis over tiles, as four members share a wave), ``__shfl(x, l, 16)`` as the gather ``x[l]``,
    ``__shfl_xor(x, mask, 16)`` as ``x[lane ^ mask]``, the same kInf, trip counts, butterfly minimum and tie rule.
    ``D`` is one ``(K, K)`` tile (rows: centroids, columns: member rows) or a stack ``(B, K, K)``; returns ``pcol``
    ``(16,)`` or ``(B, 16)``: the centroid matched to the column on every lane, -1 where none is."""
    D = np.asarray(D, dtype=np.float64)
    single = D.ndim == 2
    D = D[None] if single else D
    B = D.shape[0]
    cost = np.ones((B, LANES, LANES))  # (the pads of a tile hold 1 - 0; no open lane reads them)
    cost[:, :K, :K] = D
    lane = np.broadcast_to(np.arange(LANES), (B, LANES))
    bi = np.arange(B)[:, None]

    def shfl(x, src):
        return np.take_along_axis(x, src, axis=1)

    col = lane < K
    u, v = np.zeros((B, LANES)), np.zeros((B, LANES))
    pcol = np.full((B, LANES), -1)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(K):
            minv = np.full((B, LANES), KINF)
            way, i0, j0, jend = (np.full((B, LANES), x) for x in (-1, r, -1, -1))
            used, rowin, done = np.zeros((B, LANES), bool), lane == r, np.zeros((B, LANES), bool)
            for it in range(r + 1):
                ui0 = shfl(u, i0)
                cur = cost[bi, i0, lane] - ui0 - v
                open_ = col & ~used
                better = ~done & open_ & (cur < minv)
                minv, way = np.where(better, cur, minv), np.where(better, j0, way)
                delta, j1 = np.where(open_, minv, KINF), lane.copy()
                for mask in (8, 4, 2, 1):
                    ov, oj = shfl(delta, lane ^ mask), shfl(j1, lane ^ mask)
                    take = (ov < delta) | ((ov == delta) & (oj < j1))
                    delta, j1 = np.where(take, ov, delta), np.where(take, oj, j1)
                pj1 = shfl(pcol, j1)
                go = ~done
                u = np.where(go & rowin, u + delta, u)
                v = np.where(go & used, v - delta, v)
                minv = np.where(go & ~used, minv - delta, minv)
                j0 = np.where(go, j1, j0)
                used = used | (go & (lane == j1))
                free = go & (pj1 < 0)
                jend = np.where(free, j1, jend)
                i0 = np.where(go & ~free, pj1, i0)
                rowin = rowin | (go & ~free & (lane == pj1))
                done = done | free
            jc = jend
            for it in range(r + 1):  # augment along the predecessors
                jp = shfl(way, np.where(jc < 0, 0, jc))
                pp = shfl(pcol, np.where(jp < 0, 0, jp))
                live = jc >= 0
                pcol = np.where(live & (lane == jc), np.where(jp < 0, r, pp), pcol)
                jc = np.where(live, jp, jc)
    return pcol[0] if single else pcol


def lane_permutation(pcol: np.ndarray, K: int) -> np.ndarray:
    """The kernel's hand-off of one solve: ``pm[pc] = j`` from every lane j < K whose ``pc`` lies in [0, K) (lanes in
    ascending order: where two lanes name one row, which store lands last is not specified on the device), then the rows
    left unset take the columns left over in ascending order.  Returns ``pm[:K]``, the member row of each centroid: a
    permutation whatever ``pcol`` holds."""
    pm = np.full(K, -1)
    for j in range(K):
        if 0 <= pcol[j] < K:
            pm[pcol[j]] = j
    c = 0
    for r in range(K):
        if pm[r] < 0:
            while c < K - 1 and c in pm:
                c += 1
            pm[r] = c
            c += c < K - 1
    return pm


def augmenting_paths(D):
    """A plain row-by-row Hungarian solve (rows: centroids, added in the kernel's order 0, 1, ...; potentials on rows and
    columns): ``(p, path, tree)`` with ``p[j]`` the column of row j, ``path[r]`` the number of columns on the augmenting
    path that added row r and ``tree[r]`` the number of columns its alternating tree took in before it reached a free
    one.  ``path[r] <= tree[r] <= r + 1``: the two fixed trip counts of ``stab_assign``."""
    D = np.asarray(D, dtype=np.float64)
    K = len(D)
    u, v = np.zeros(K), np.zeros(K)
    row_of = np.full(K, -1)  # the row matched to a column
    path, tree = np.zeros(K, dtype=int), np.zeros(K, dtype=int)
    for r in range(K):
        minv, way, used = np.full(K, np.inf), np.full(K, -1), np.zeros(K, bool)
        i0, j0 = r, -1
        while True:
            cur = D[i0] - u[i0] - v
            better = ~used & (cur < minv)
            minv[better], way[better] = cur[better], j0
            j1 = int(np.argmin(np.where(used, np.inf, minv)))  # (the first of equal minima, as on the device)
            delta = minv[j1]
            in_tree = np.concatenate([[r], row_of[used]])
            u[in_tree] += delta
            v[used] -= delta
            minv[~used] -= delta
            used[j1] = True
            tree[r] += 1
            j0 = j1
            if row_of[j1] < 0:
                break
            i0 = row_of[j1]
        while j0 >= 0:
            j1 = way[j0]
            row_of[j0] = r if j1 < 0 else row_of[j1]
            path[r] += 1
            j0 = j1
    p = np.empty(K, dtype=np.int32)
    p[row_of] = np.arange(K)
    return p, path, tree


def lane_stability(signatures, errors=None, max_rounds: int = 20) -> SimpleNamespace:
    """``stability_kernel`` with ``lane_assign`` in the place of the optimal assignment and the kernel's own handling of
    what is not finite (a norm of 0 or NaN gives a NaN unit row; ``!(d >= b)`` and ``!(z >= lo)`` let a NaN through):
    what the device does on input that the contract excludes.  Assignments, rounds and the scores only."""
    s = np.asarray(signatures, dtype=np.float64)
    M, K, V = s.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        u = s / np.sqrt((s * s).sum(axis=2, keepdims=True))
        xx = (u * u).sum(axis=2)
        errors = np.zeros(M) if errors is None else np.asarray(errors, dtype=np.float64)
        best = 0
        for m in range(1, M):
            if errors[m] < errors[best]:
                best = m
        c = u[best].copy()
        P = np.zeros((M, K), dtype=np.int32)
        n_rounds, converged = 0, False
        sums = np.zeros((K, V))
        for t in range(1, max_rounds + 1):
            pcol = lane_assign(1.0 - np.einsum("jv,miv->mji", c, u), K)
            new = np.stack([lane_permutation(pcol[m], K) for m in range(M)]).astype(np.int32)
            changed = t == 1 or not np.array_equal(new, P)
            P = new
            n_rounds = t
            if not changed:
                converged = True
                break
            sums = np.zeros((K, V))
            for m in range(M):
                sums += u[m][P[m]]
            if t == max_rounds:
                break
            c = sums / np.sqrt((sums * sums).sum(axis=1, keepdims=True))
        a, b, z = np.zeros((M, K)), np.full((M, K), np.nan), np.ones((M, K))
        for m in range(M):
            for j in range(K):
                i = P[m, j]
                x = u[m, i] @ sums.T
                a[m, j] = 1.0 - (x[j] - xx[m, i]) / (M - 1)
                for k in range(K):
                    d = 1.0 - x[k] / M
                    if k != j and not d >= b[m, j]:
                        b[m, j] = d
                if K > 1:
                    z[m, j] = (b[m, j] - a[m, j]) / (a[m, j] if a[m, j] > b[m, j] else b[m, j])
        cluster = z.sum(axis=0) / M
        lo = cluster[0]
        for x in cluster:
            if lo == lo and not x >= lo:
                lo = x
    return SimpleNamespace(assignments=P, n_rounds=n_rounds, converged=converged, a=a, b=b, silhouette=z, cluster_stability=cluster,
                           stability_mean=float(cluster.sum() / K), stability_min=float(lo))


# ------------------------------------------------------------------ constructed instances: any cost tile through the API
def block_group(A_list, V: int, equal_norms: bool = False):
    """A group ``(1 + len(A_list), K, V)`` and its errors whose first round solves the assignment on a prescribed tile.
    Member 0, the anchor (error 0, the others 1), has the indicators of K disjoint blocks of ``w = V // K`` features as its
    rows; row i of member 1 + n carries ``A_list[n][i, j]`` on block j.  Then ``c[j] . u[i] = A[i, j] / |A[i]|`` and round
    1 solves ``D[j, i] = 1 - A[i, j] / |A[i]|`` for member 1 + n -- any non-negative A with no zero row.

    The division by ``|A[i]|`` scales every column of the tile by its own factor and so moves the optimum.
    ``equal_norms`` undoes that: an indicator sees only the sum over its block, so moving weight inside every block on to
    its first feature (``1 + (w - 1) g`` against ``1 - g`` times the even share, 0 <= g <= 1) raises the norm of a row,
    by up to ``sqrt(w)``, and changes no dot product with the anchor.  All rows of a member are brought to the norm n of
    its longest row: round 1 then solves ``1 - A[i, j] / n``, which has the optimum, the augmenting paths and the ties of
    ``-A^T`` exactly."""
    A_list = [np.asarray(A, dtype=np.float64) for A in A_list]
    K = A_list[0].shape[0]
    w = V // K
    assert w >= 1 and all(A.shape == (K, K) and (A >= 0).all() and (A.sum(axis=1) > 0).all() for A in A_list)
    blocks = np.zeros((K, V))
    for j in range(K):
        blocks[j, j * w : (j + 1) * w] = 1.0
    members = []
    for A in A_list:
        rows = A @ blocks / np.sqrt(w)
        if equal_norms:
            n2 = (A * A).sum(axis=1)
            g = np.sqrt((n2.max() / n2 - 1.0) / (w - 1))
            assert (g <= 1.0).all(), "rows too unequal for blocks of this width"
            spread = np.tile(1.0 - g[:, None], (1, V))
            spread[:, np.arange(K) * w] = 1.0 + (w - 1) * g[:, None]
            rows = rows * spread
        members.append(rows)
    sigs = np.stack([blocks] + members)
    errors = np.ones(len(sigs))
    errors[0] = 0.0
    return sigs, errors


def chain_tile(K: int) -> np.ndarray:
    """``D[j, i] = ((i + j) / (2 K - 2))^2 / 8``.  For every r the cheapest assignment of rows 0 .. r is the
    anti-diagonal i + j = r and no other: the mean of i + j is at least r, with equality on columns 0 .. r alone, and the
    square is strictly convex.  Adding row r therefore moves every matched row one column up: its augmenting path passes
    through all r + 1 columns, the most there are."""
    s = np.add.outer(np.arange(K), np.arange(K)) / max(2 * K - 2, 1)
    return s * s / 8.0


def machol_wien(K: int, seed: int) -> np.ndarray:
    """A (K, K) for ``block_group(..., equal_norms=True)``: ``1 - D^T`` of the Machol-Wien costs
    ``D[j, i] = (j + 1)(i + 1) / K^2`` plus ``1e-3 * rng.random``.  Every row of D has its minimum in column 0; the
    optimum is the anti-diagonal."""
    k = np.arange(1, K + 1)
    D = np.outer(k, k) / (K * K) + 1e-3 * np.random.default_rng(seed).random((K, K))
    return np.maximum(1.0 - D.T, 0.0)


def long_path(K: int, seed: int) -> np.ndarray:
    """A (K, K) for ``block_group(..., equal_norms=True)``: ``1 - D^T`` of ``chain_tile(K)`` plus ``1e-6 * rng.random``,
    noise far inside the gaps of that tile (2 / (8 (2 K - 2)^2) >= 2.7e-4).  With equal norms the tile solved is a positive
    multiple of D plus a constant, so no search is needed for the longest path a realisable instance can have: it is K."""
    return 1.0 - (chain_tile(K) + 1e-6 * np.random.default_rng(seed).random((K, K))).T


def near_tie(K: int, seed: int, noise: float = 1e-4) -> np.ndarray:
    """A (K, K) for ``block_group(..., equal_norms=True)`` with two equal optima but for noise: column 1 of a random A
    (entries in [0.5, 1]) is a copy of column 0, so centroids 0 and 1 see every member row alike, plus
    ``noise * (1 + q[i] / K)`` in row i, q a random permutation.  Exchanging the rows of centroids 0 and 1 then costs
    between ``noise / (K n)`` and ``noise / n``, n <= sqrt(K) the common norm: inside [1e-6, 1e-4] for K <= 16."""
    rng = np.random.default_rng(seed)
    A = 0.5 + 0.5 * rng.random((K, K))
    A[:, 1] = A[:, 0] + noise * (1.0 + rng.permutation(K) / K)
    return A


def exact_tie(K: int) -> np.ndarray:
    """A (K, K) for ``block_group`` whose rows 0 and 1 are equal: two member rows of the same bits, so every assignment
    has a twin of exactly the same cost."""
    A = 0.1 + np.random.default_rng(K).random((K, K))
    A[1] = A[0]
    return A


def random_dense(K: int, M: int, seed: int):
    """A group of M members and its errors: M - 1 members ``A = rng.random((K, K))`` behind one block anchor, V = 96."""
    rng = np.random.default_rng(seed)
    return block_group([rng.random((K, K)) for _ in range(M - 1)], 96)



HARD_FAMILIES = {"machol_wien": machol_wien, "long_path": long_path, "near_tie": near_tie}
HARD_KS = (2, 3, 8, 15, 16)
HARD_VS = (96, 83)
DENSE_CASES = ((5, 65), (16, 65), (16, 17))  # (K, M): five passes with one member in the last; one member in a second slot
DENSE_MAX_ROUNDS = 40


@functools.lru_cache(maxsize=None)
def hard_case(family: str, K: int, V: int):
    """``(signatures, errors, replica result)`` of one constructed pair: the block anchor and one member of ``family``.
    ``family`` "dense" takes M in the place of V.  Shared between the tests and read-only."""
    if family == "dense":
        sigs, errors = random_dense(K, V, seed=0)
        want = stability(sigs, errors, DENSE_MAX_ROUNDS)
    else:
        sigs, errors = block_group([HARD_FAMILIES[family](K, seed=0)], V, equal_norms=True)
        want = stability(sigs, errors)
    sigs.setflags(write=False)
    errors.setflags(write=False)
    return sigs, errors, want


def first_tile(want: SimpleNamespace, m: int = 1) -> np.ndarray:
    """The cost tile of member m in round 1 of a replica result."""
    return 1.0 - want.unit[want.anchor] @ want.unit[m].T


def greedy_is_optimal(D: np.ndarray) -> bool:
    """Whether every row's own minimum is the optimal assignment (then a solver needs no augmenting path at all)."""
    return np.array_equal(D.argmin(axis=1), assign(D, margin=False)[0])
