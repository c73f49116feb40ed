"""Host replica of ``sal.assign_signatures`` with candidate sets, required signatures and the re-addition pass (DESIGN.md
section 14.1), on the functions of ``tests/_refit_ref.py`` and ``tests/_assign_ref.py``.

Per problem (sample n): C_n is the candidate set, R_n, a subset of it, the required set.  Phase 0: A = C_n, h_k = sum(x) / |C_n|
on C_n and exactly 0.0 elsewhere, solved as section 14 defines a solve.  Backward rounds as ``_assign_ref.assign``, with the
protected set starting as R_n.  Re-addition pass (``readd``), after the rounds have ended with (A, h, f): the pool is
C_n \\ A, each member tried at most once; at the accepted h every pool member has the update factor
u_k = sum_v W[k, v] x_v / (h W)_v (the step's own factor); the candidate c is the untried pool member of largest u_k, taken
in ascending k with a strict comparison from -inf (lowest index on equal values, a NaN never wins); without one, or unless
u_c > 1, the procedure ends; trial: h with entry c set to sum(x) / |C_n|, solved with A + {c}; if f - f' > max_kl_increase
(false for a NaN) the trial's h, f, A are accepted; either way c is tried.

``trials[p]`` records every decision with what isolates it.  A backward trial: kind "remove", candidate, value, runner (the
runner-up's h, inf without one), delta = f' - f, accepted.  A selection of the re-addition pass: kind "select", candidate (-1
without one), value = u_c, runner (the runner-up's u, -inf without one), go; if it goes, the trial follows as kind "add" with
candidate, delta = f - f', accepted.
"""

import functools
from types import SimpleNamespace

import numpy as np

import _assign_ref as aref
import _refit_ref as ref

EPSILON = ref.EPSILON


def masks(candidates, required, N, K):
    """The two sets as (N, K) bool arrays; ``ValueError`` for what the contract refuses."""
    C = np.ones((N, K), dtype=bool) if candidates is None else np.broadcast_to(np.asarray(candidates, dtype=bool), (N, K)).copy()
    R = np.zeros((N, K), dtype=bool) if required is None else np.broadcast_to(np.asarray(required, dtype=bool), (N, K)).copy()
    if not C.any(axis=1).all():
        raise ValueError("a sample has no candidate signature")
    if (R & ~C).any():
        raise ValueError("a required signature is not a candidate")
    return C, R


def update_factors(x, W, h):
    """u[p, k] = sum_v W[k, v] x[p, v] / (h W)[p, v]: what ``_refit_ref.step`` multiplies h by."""
    return np.einsum("pv,kv->pk", x / ref._wh(h, W), W)


def largest(u, eligible):
    """(index, value, runner-up value) of the largest eligible entry, lowest index on equal values; index -1 without one."""
    best, value, runner = -1, -np.inf, -np.inf
    for k in np.flatnonzero(eligible):
        if u[k] > value:
            best, value, runner = int(k), u[k], value
        elif u[k] > runner:
            runner = u[k]
    return best, value, runner


def assign(X, W, max_kl_increase=1.92, min_iterations=500, max_iterations=10000, conv_test_freq=10, tol=1e-7, dtype=np.float64, perm=None,
           candidates=None, required=None, readd=False):
    aref.check(max_iterations, conv_test_freq, max_kl_increase)
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    if perm is not None:
        X, W = X[:, perm], W[:, perm]
    x = np.maximum(X, EPSILON).astype(dtype)
    W = W.astype(dtype)
    P, K = x.shape[0], W.shape[0]
    C, R = masks(candidates, required, P, K)
    h0 = x.sum(axis=1) / C.sum(axis=1)
    h = np.where(C, h0[:, None], dtype(0.0)).astype(dtype)
    accepted = h.copy()
    active = C.copy()
    protected = R.copy()
    tried = ~C
    mode = np.zeros(P, dtype=np.int64)  # 0: phase 0, 1: a backward trial, 2: finished, 3: a re-addition trial, 4: waits for its candidate
    fresh = np.zeros(P, dtype=bool)
    itl = np.zeros(P, dtype=np.int64)
    cand = np.zeros(P, dtype=np.int64)
    prev = np.zeros(P, dtype=dtype)
    f = np.zeros(P, dtype=dtype)
    n_trials = np.zeros(P, dtype=np.int64)
    n_iterations = np.zeros(P, dtype=np.int64)
    converged = np.ones(P, dtype=bool)
    removal_round = np.full((P, K), -1, dtype=np.int64)
    readd_round = np.full((P, K), -1, dtype=np.int64)
    kl_increase = np.full((P, K), np.nan, dtype=dtype)
    kl_decrease = np.full((P, K), np.nan, dtype=dtype)
    dense = SimpleNamespace(exposures=np.zeros((P, K), dtype=dtype), reconstruction_errors=np.zeros(P, dtype=dtype),
                            n_iterations=np.zeros(P, dtype=np.int64), converged=np.zeros(P, dtype=bool))
    trials = [[] for _ in range(P)]
    g = 0
    while True:
        if g % conv_test_freq == 0:
            repass = False
            while True:
                cur = ref.objective(x, W, h)
                select = mode == 4
                todo = (mode != 2) & ~select & (fresh | (not repass))
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel = np.abs(prev - cur) / np.abs(prev)
                hit = todo & (itl > 0) & (itl >= min_iterations) & (rel < tol)
                stop = hit | (todo & (itl == max_iterations))
                prev = np.where(todo, cur, prev)
                fresh[:] = False
                for p in np.flatnonzero(stop):
                    n_iterations[p] += itl[p]
                    converged[p] &= bool(hit[p])
                    add = mode[p] == 3
                    if mode[p] == 0:
                        dense.exposures[p], dense.reconstruction_errors[p] = h[p], cur[p]
                        dense.n_iterations[p], dense.converged[p] = itl[p], hit[p]
                        accept = True
                    elif add:
                        c = cand[p]
                        delta = f[p] - cur[p]
                        accept = bool(delta > max_kl_increase)
                        kl_decrease[p, c] = delta
                        trials[p][-1].update(delta=delta, accepted=accept)
                        tried[p, c] = True
                        if accept:
                            active[p, c] = True
                            readd_round[p, c] = n_trials[p]
                        n_trials[p] += 1
                    else:
                        c = cand[p]
                        delta = cur[p] - f[p]
                        accept = bool(delta <= max_kl_increase)
                        kl_increase[p, c] = delta
                        trials[p][-1].update(delta=delta, accepted=accept)
                        if accept:
                            active[p, c] = False
                            removal_round[p, c] = n_trials[p]
                        else:
                            protected[p, c] = True
                        n_trials[p] += 1
                    if accept:
                        f[p], accepted[p] = cur[p], h[p]
                    else:
                        h[p] = accepted[p]
                    c, value, runner = aref.candidate(h[p], active[p] & ~protected[p])
                    if add or c < 0 or active[p].sum() == 1:
                        mode[p] = 4 if readd else 2
                    else:
                        trials[p].append(dict(kind="remove", candidate=c, value=value, runner=runner))
                        cand[p], mode[p], itl[p], fresh[p] = c, 1, 0, True
                        h[p, c] = 0.0
                if select.any():
                    # (h is the accepted h in these problems, and nothing above touched them in this pass)
                    u = update_factors(x, W, h)
                    for p in np.flatnonzero(select):
                        c, value, runner = largest(u[p], ~active[p] & ~tried[p])
                        go = bool(c >= 0 and value > 1.0)
                        trials[p].append(dict(kind="select", candidate=c, value=value, runner=runner, go=go))
                        if go:
                            trials[p].append(dict(kind="add", candidate=c))
                            cand[p], mode[p], itl[p], fresh[p] = c, 3, 0, True
                            h[p, c] = h0[p]
                        else:
                            mode[p] = 2
                if not (fresh.any() or (mode == 4).any()):
                    break
                repass = True
        if (mode == 2).all():
            break
        live = mode != 2
        h = np.where(live[:, None], np.where(h == 0.0, h, ref.step(x, W, h)), h)
        itl[live] += 1
        g += 1
    return SimpleNamespace(exposures=h, active=active, reconstruction_errors=f, removal_round=removal_round, kl_increase=kl_increase,
                           readd_round=readd_round, kl_decrease=kl_decrease, n_trials=n_trials, n_iterations=n_iterations, converged=converged,
                           dense=dense, trials=trials, candidates=C, required=R)


def on_subcatalogue(X, W, candidates, **kw):
    """``_assign_ref.assign`` row by row on the sub-catalogue ``W[C_n]``, its results scattered back to K columns: what a
    restriction to C_n has to equal (backward rounds only, no required set)."""
    X = np.asarray(X, dtype=np.float64)
    P, K = X.shape[0], W.shape[0]
    C, _ = masks(candidates, None, P, K)
    dtype = kw.get("dtype", np.float64)
    out = SimpleNamespace(exposures=np.zeros((P, K), dtype=dtype), active=np.zeros((P, K), dtype=bool), reconstruction_errors=np.zeros(P, dtype=dtype),
                          removal_round=np.full((P, K), -1, dtype=np.int64), kl_increase=np.full((P, K), np.nan, dtype=dtype),
                          n_trials=np.zeros(P, dtype=np.int64), n_iterations=np.zeros(P, dtype=np.int64), converged=np.zeros(P, dtype=bool),
                          dense=SimpleNamespace(exposures=np.zeros((P, K), dtype=dtype), reconstruction_errors=np.zeros(P, dtype=dtype),
                                                n_iterations=np.zeros(P, dtype=np.int64), converged=np.zeros(P, dtype=bool)))
    for p in range(P):
        idx = np.flatnonzero(C[p])
        sub = aref.assign(X[p:p + 1], W[idx], **kw)
        for name in ("exposures", "active", "removal_round", "kl_increase"):
            getattr(out, name)[p, idx] = getattr(sub, name)[0]
        out.dense.exposures[p, idx] = sub.dense.exposures[0]
        for name in ("reconstruction_errors", "n_trials", "n_iterations", "converged"):
            getattr(out, name)[p] = getattr(sub, name)[0]
        for name in ("reconstruction_errors", "n_iterations", "converged"):
            getattr(out.dense, name)[p] = getattr(sub.dense, name)[0]
    return out


def isolation(runs, max_kl_increase, rel=1e-6):
    """Per problem: do the replicas `runs` take the same decisions, and is every one of them isolated?  Every threshold
    comparison (f' - f and f - f' against max_kl_increase) clears it by rel * max(1, |threshold|); every u_c clears 1 by rel;
    every arg-min winner is bit-equal to EPSILON or a relative rel below its runner-up, every arg-max winner a relative rel
    above its runner-up.  Also returns the smallest threshold margin and the smallest margin of a u_c about 1."""
    P = len(runs[0].trials)
    scale = max(1.0, abs(max_kl_increase))
    ok = np.ones(P, dtype=bool)
    margin, umargin = np.inf, np.inf

    def key(t):
        return (t["kind"], t["candidate"], t.get("accepted"), t.get("go"))

    for p in range(P):
        first = [key(t) for t in runs[0].trials[p]]
        for run in runs:
            mine = run.trials[p]
            if [key(t) for t in mine] != first:
                ok[p] = False
            for t in mine:
                good = True
                if t["kind"] in ("remove", "add"):
                    m = abs(float(t["delta"]) - max_kl_increase) / scale
                    margin = min(margin, m)
                    good = m >= rel
                if t["kind"] == "remove":
                    good = good and (float(t["value"]) == EPSILON or float(t["value"]) <= float(t["runner"]) * (1 - rel))
                if t["kind"] == "select" and t["candidate"] >= 0:
                    um = abs(float(t["value"]) - 1.0)
                    umargin = min(umargin, um)
                    good = um >= rel and float(t["runner"]) <= float(t["value"]) * (1 - rel)
                if not good:
                    ok[p] = False
    return ok, margin, umargin


# The cases of tests/test_gpu_assign_masks.py, whose isolation tests/test_assign_masks_host.py shows on the CPU:
# (P, K, V, seed, sets, readd, max_kl_increase).  K = 1, 2, 3, both sides of 16, 33 (one bit into the second mask word), 64, 96;
# V = 7 and 96; P = one problem, one tile, the tile boundary, a partial third tile.  `sets`:
#   "random"    per-sample candidate sets, every signature in with probability 1 / 2 (and one at random always in)
#   "shared"    one (K,) set for every sample, built the same way
#   "single"    per-sample sets of size 1
#   "word"      signatures 0..31: the set ends exactly on the first mask word
#   "word2"     signatures 32..63: the set fills exactly the second mask word
#   "prefix"    signatures 0..32 of 40: the sub-catalogue has the same KT and keeps every signature in its position
#   "required"  "random", and of each sample's candidates a random third is required (at least one)
#   "edge"      "random", and every sample holds the last signature and the first one of the last mask word, 32 floor((K - 1) / 32)
#               (tests/test_gpu_family_edges.py)
# At 20-step solves and the default threshold no re-addition trial of these inputs is accepted (the backward rounds only
# remove what costs less than 1.92, and a signature that comes back gains about what it cost); the thresholds 0.1 and -0.01
# are those at which the K = 33 and K = 96 cases accept one each, still isolated.
CASES = [
    (40, 1, 96, 0, "shared", True, 1.92),
    (1, 2, 7, 0, "single", True, 1.92),
    (40, 3, 7, 0, "random", True, 1.92),
    (17, 16, 96, 0, "required", True, 1.92),
    (16, 17, 96, 0, "random", True, 1.92),
    (17, 33, 96, 0, "word", True, 0.1),
    (16, 64, 96, 0, "word2", False, 1.92),
    (16, 96, 96, 0, "required", True, -0.01),
    (40, 16, 96, 0, "shared", False, 1.92),
    (17, 64, 7, 0, "single", True, 1.92),
    (17, 40, 96, 0, "prefix", False, 1.92),
]
FIXED = dict(min_iterations=20, max_iterations=20, conv_test_freq=5)  # every solve is 20 steps long
PERM_SEED = 7
PLANTED_SEED = 94  # of _assign_ref.planted_catalogue: the seed in 0..99 whose re-addition pass accepts two signatures
# Largest deviation of the two float64 feature orders from the longdouble replica over CASES, measured on the CPU
# (tests/test_assign_masks_host.py asserts each case stays within them); the device is held to 16 x these.
H_SPREAD = 1.7e-14  # measured 1.62e-14 (P = 16, K = 96): |dH| / max(H_ld, EPSILON) on the support
F_SPREAD = 3.5e-16  # measured 3.46e-16 (P = 16, K = 64): |df|, |d kl_increase|, |d kl_decrease| relative to the row's sum_v |x log(x / wh)| + x + wh


def case_sets(P, K, seed, sets):
    """(candidates, required) of a case: (P, K) or (K,) bool arrays, or None."""
    rng = np.random.default_rng(1000 + seed)

    def random_rows(n):
        C = rng.random((n, K)) < 0.5
        C[np.arange(n), rng.integers(0, K, size=n)] = True
        return C

    if sets == "shared":
        return random_rows(1)[0], None
    if sets == "single":
        C = np.zeros((P, K), dtype=bool)
        C[np.arange(P), rng.integers(0, K, size=P)] = True
        return C, None
    if sets in ("word", "word2"):
        C = np.zeros(K, dtype=bool)
        C[32:64] = sets == "word2"
        C[0:32] = sets == "word"
        return C, None
    if sets == "prefix":
        return np.arange(K) < 33, None
    C = random_rows(P)
    if sets == "random":
        return C, None
    if sets == "edge":
        C[:, [K - 1, 32 * ((K - 1) // 32)]] = True
        return C, None
    R = np.zeros((P, K), dtype=bool)
    for p in range(P):
        idx = np.flatnonzero(C[p])
        R[p, rng.choice(idx, size=max(1, idx.size // 3), replace=False)] = True
    return C, R


def case_inputs(P, K, V, seed, sets, readd, thr):
    """(X, W, keyword arguments of the masked call) of a case; the last rows of X are near-empty."""
    X, W = ref.poisson_catalogue(P, K, V=V, seed=seed, zero_heavy=min(3, P - 1))
    C, R = case_sets(P, K, seed, sets)
    return X, W, dict(max_kl_increase=thr, candidates=C, required=R, readd=readd)


def three_runs(X, W, solve=FIXED, **kw):
    """The float64 replica, the float64 replica in another feature order and the longdouble replica of one call."""
    perm = np.random.default_rng(PERM_SEED).permutation(X.shape[1])
    return assign(X, W, **solve, **kw), assign(X, W, perm=perm, **solve, **kw), assign(X, W, dtype=np.longdouble, **solve, **kw)


@functools.lru_cache(maxsize=None)
def case_replicas(*case):
    """A case's inputs, its call's keyword arguments, its three host runs and their isolation, computed once and shared by the
    tests that need them (never modified)."""
    X, W, kw = case_inputs(*case)
    runs = three_runs(X, W, **kw)
    return X, W, kw, runs, isolation(runs, kw["max_kl_increase"])


def row_scale(X, W, H):
    x = np.maximum(X, EPSILON)
    wh = np.asarray(H, dtype=np.float64) @ W
    return (np.abs(x * np.log(x / wh)) + x + wh).sum(axis=1)


def deviations(got, ld, scale, rows=None):
    """(H, f) deviations of a run from the longdouble replica `ld` on `rows` (all by default), where both have the same
    support: |dH| / max(H_ld, EPSILON) on the support; the objective, kl_increase and kl_decrease relative to `scale`."""
    rows = np.arange(ld.exposures.shape[0]) if rows is None else rows
    H_ld = ld.exposures[rows]
    dH = float((np.abs(got.exposures[rows] - H_ld) / np.maximum(H_ld, EPSILON))[ld.active[rows]].max(initial=0.0))
    dF = float((np.abs(got.reconstruction_errors[rows] - ld.reconstruction_errors[rows]) / scale[rows]).max(initial=0.0))
    for name in ("kl_increase", "kl_decrease"):
        mine, theirs = getattr(got, name), getattr(ld, name)
        if mine is None:
            continue
        tested = ~np.isnan(theirs[rows].astype(np.float64))
        dF = max(dF, float((np.abs(mine[rows] - theirs[rows]) / scale[rows, None])[tested].max(initial=0.0)))
    return dH, dF


def host_spread(X, W, runs, rows=None):
    """(scale, H spread, f spread): the two float64 runs against the longdouble run."""
    a, b, ld = runs
    scale = row_scale(X, W, ld.exposures)
    da, db = deviations(a, ld, scale, rows), deviations(b, ld, scale, rows)
    return scale, max(da[0], db[0]), max(da[1], db[1])
